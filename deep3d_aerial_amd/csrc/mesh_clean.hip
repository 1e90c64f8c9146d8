// Mesh cleaning: adjacency, connected components, removal of small components, Laplacian smoothing.  The
// semantics are this project's (deep3d_aerial_amd/mesh.py states them, include/deep3d_planesweep.h too).
//
// adjacency:  one lane per face adds 2 entries per distinct edge (integer atomicAdd on the row counts), a scan gives the row
//             starts, a second pass scatters the entries (the atomic's return value is the slot), and one lane per vertex sorts
//             its row in registers (bitonic, up to 32 entries), drops the duplicates, tests the multiplicities (manifold: 2)
//             and writes the distinct neighbours in place.  Longer rows go to a list that workgroups walk: a rank sort and a
//             scan of the run starts.  A scan of the distinct counts and a copy give the CSR.  Every row is sorted, so the
//             arrival order of the scatter never reaches the output.
// components: parent[v] = v; hooking (one lane per face, geom_hook of its corners) and full pointer jumping in separate
//             launches until a hooking launch changes nothing; the host reads one flag per round.  The fixed point is the
//             smallest vertex index of each component.
// stats:      per-component face counts (atomicAdd) and boxes (atomicMin / atomicMax of dsm_key), each wave folding a run of
//             equal labels before its atomics; the box of the referenced vertices by the same keys.
// filter:     a keep flag per face, a scan, a scatter of the kept faces in input order and the referenced flags (then
//             d3d_mesh_compact).
// smooth:     one lane per vertex walks its CSR row in order (fp32 sums, no contraction); one launch per iteration, ping-pong.
// Integer atomics only; every float result is a fixed-order computation, so nothing depends on the order lanes run in.
#include <climits>
#include <cmath>
#include <cstdint>

#include "common.h"
#include "geom_shared.h"

namespace d3d {

constexpr int MC_BLOCK = 256;
constexpr int MC_ROW_REG = 32;       // rows of at most this many entries are sorted in registers
constexpr int MC_SLOW_GRID = 256;    // workgroups walking the list of longer rows
constexpr int MC_CHUNK = 64 * 64;    // faces / vertices per wave in the stats passes (64 steps of 64)
constexpr long long MC_MAX_ENTRIES = (1ll << 31) - 1;

// ---------------------------------------------------------------------------------------------------------------------------
// adjacency
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MC_BLOCK) void mc_count_kernel(const int* __restrict__ faces, long m, long long n, int* __restrict__ cnt) {
    const long f = (long)blockIdx.x * MC_BLOCK + threadIdx.x;
    int a, b, c;
    if (f >= m || !geom_face<false>(faces, f, n, &a, &b, &c)) return;
    int x[3], y[3];
    const int ne = geom_face_edges(a, b, c, x, y);
#pragma unroll
    for (int e = 0; e < 3; ++e)
        if (e < ne) {
            atomicAdd(cnt + x[e], 1);
            atomicAdd(cnt + y[e], 1);
        }
}

__global__ __launch_bounds__(MC_BLOCK) void mc_scatter_kernel(const int* __restrict__ faces, long m, long long n, const int* __restrict__ start,
                                                              int* __restrict__ fill, int* __restrict__ ent) {
    const long f = (long)blockIdx.x * MC_BLOCK + threadIdx.x;
    int a, b, c;
    if (f >= m || !geom_face<false>(faces, f, n, &a, &b, &c)) return;
    int x[3], y[3];
    const int ne = geom_face_edges(a, b, c, x, y);
#pragma unroll
    for (int e = 0; e < 3; ++e)
        if (e < ne) {
            ent[(long)start[x[e]] + atomicAdd(fill + x[e], 1)] = y[e];
            ent[(long)start[y[e]] + atomicAdd(fill + y[e], 1)] = x[e];
        }
}

// Sorts the L <= N entries of row in registers (INT_MAX pads: no vertex index reaches it), writes the distinct ones back to
// the start of the row; returns their count, *fixed: some neighbour does not occur exactly twice, or there is none.
template <int N>
__device__ __forceinline__ int mc_row_registers(int* __restrict__ row, int L, bool* fixed) {
    int a[N];
#pragma unroll
    for (int k = 0; k < N; ++k) a[k] = k < L ? row[k] : INT_MAX;
#pragma unroll
    for (int size = 2; size <= N; size <<= 1)
#pragma unroll
        for (int stride = size >> 1; stride > 0; stride >>= 1)
#pragma unroll
            for (int i = 0; i < N; ++i) {
                const int j = i ^ stride;
                if (j > i) {
                    const int lo = min(a[i], a[j]), hi = max(a[i], a[j]);
                    const bool up = (i & size) == 0;
                    a[i] = up ? lo : hi;
                    a[j] = up ? hi : lo;
                }
            }
    int u = 0;
    bool fx = L == 0;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        if (a[k] == INT_MAX || (k > 0 && a[k] == a[k - 1])) continue;
        const bool twice = k + 1 < N && a[k + 1] == a[k] && (k + 2 >= N || a[k + 2] != a[k]);
        fx |= !twice;
        row[u++] = a[k];
    }
    *fixed = fx;
    return u;
}

__global__ __launch_bounds__(MC_BLOCK) void mc_rows_kernel(const int* __restrict__ start, const int* __restrict__ cnt, long long n,
                                                           int* __restrict__ ent, int* __restrict__ ucnt, unsigned char* __restrict__ fixed,
                                                           int* __restrict__ long_list, int* __restrict__ n_long) {
    const long v = (long)blockIdx.x * MC_BLOCK + threadIdx.x;
    if (v >= n) return;
    const int L = cnt[v];
    if (L > MC_ROW_REG) {
        long_list[atomicAdd(n_long, 1)] = (int)v;   // the list's order does not matter: each row is its own
        return;
    }
    bool fx;
    const int u = L <= 16 ? mc_row_registers<16>(ent + start[v], L, &fx) : mc_row_registers<MC_ROW_REG>(ent + start[v], L, &fx);
    ucnt[v] = u;
    fixed[v] = fx ? 1 : 0;
}

// One workgroup per long row: rank sort into srt (rank = entries below + equal entries before), then the run starts
// scanned into the distinct neighbours at the start of the row.
__global__ __launch_bounds__(MC_BLOCK) void mc_rows_slow_kernel(const int* __restrict__ start, const int* __restrict__ cnt,
                                                                const int* __restrict__ long_list, const int* __restrict__ n_long,
                                                                int* __restrict__ ent, int* __restrict__ srt, int* __restrict__ ucnt,
                                                                unsigned char* __restrict__ fixed) {
    __shared__ int lds[MC_BLOCK / 64];
    const int nl = *n_long;
    for (int q = blockIdx.x; q < nl; q += gridDim.x) {
        const int v = long_list[q];
        const long s = start[v];
        const int L = cnt[v];
        int* row = ent + s;
        int* out = srt + s;
        for (int i = threadIdx.x; i < L; i += MC_BLOCK) {
            const int x = row[i];
            int r = 0;
            for (int j = 0; j < L; ++j) {
                const int y = row[j];
                r += (y < x || (y == x && j < i)) ? 1 : 0;
            }
            out[r] = x;
        }
        __syncthreads();
        int carry = 0;
        bool fx = false;
        for (int base = 0; base < L; base += MC_BLOCK) {
            const int k = base + threadIdx.x;
            int x = 0;
            bool first = false;
            if (k < L) {
                x = out[k];
                first = k == 0 || out[k - 1] != x;
                if (first) fx |= !(k + 1 < L && out[k + 1] == x && (k + 2 >= L || out[k + 2] != x));
            }
            int total;
            const int ex = block_exclusive<int>(first ? 1 : 0, lds, &total);
            if (first) row[carry + ex] = x;   // row is only read before the barrier above
            carry += total;
        }
        fx = __syncthreads_or(fx ? 1 : 0) != 0;
        if (threadIdx.x == 0) {
            ucnt[v] = carry;
            fixed[v] = fx ? 1 : 0;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(MC_BLOCK) void mc_csr_kernel(const int* __restrict__ start, const int* __restrict__ ucnt,
                                                          const int* __restrict__ uoff, const long long* __restrict__ total, long long n,
                                                          const int* __restrict__ ent, long long* __restrict__ offset, int* __restrict__ nbr) {
    const long v = (long)blockIdx.x * MC_BLOCK + threadIdx.x;
    if (v > n) return;
    if (v == n) {
        offset[n] = *total;
        return;
    }
    const long s = start[v], o = uoff[v];
    const int u = ucnt[v];
    offset[v] = o;
    for (int k = 0; k < u; ++k) nbr[o + k] = ent[s + k];
}

// ---------------------------------------------------------------------------------------------------------------------------
// components
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MC_BLOCK) void mc_hook_kernel(const int* __restrict__ faces, long m, long long n, int* parent, int* changed) {
    const long f = (long)blockIdx.x * MC_BLOCK + threadIdx.x;
    int a, b, c;
    if (f >= m || !geom_face<false>(faces, f, n, &a, &b, &c)) return;
    const int pa = parent[a], pb = parent[b], pc = parent[c];   // one snapshot for both hooks
    geom_hook(parent, pa, pb, changed);
    geom_hook(parent, pa, pc, changed);
}

// ---------------------------------------------------------------------------------------------------------------------------
// component stats
// ---------------------------------------------------------------------------------------------------------------------------
// Each wave takes MC_CHUNK consecutive faces.  The faces whose label is lane 0's are counted together and folded into a
// running count while that label repeats; one atomicAdd per run, one per face of any other label.  The referenced flags are
// idempotent stores.
__global__ __launch_bounds__(MC_BLOCK) void mc_face_stats_kernel(const int* __restrict__ faces, long m, long long n, const int* __restrict__ label,
                                                                 int* __restrict__ face_count, int* __restrict__ referenced) {
    const int lane = threadIdx.x & 63;
    const long base = ((long)blockIdx.x * (MC_BLOCK / 64) + (threadIdx.x >> 6)) * MC_CHUNK;
    int cur = -1, run = 0;
    for (int step = 0; step < MC_CHUNK / 64; ++step) {
        const long f = base + step * 64 + lane;
        if (base + step * 64 >= m) break;   // wave-uniform
        int a, b, c;
        const bool ok = f < m && geom_face<false>(faces, f, n, &a, &b, &c);
        const int r = ok ? label[a] : -1;
        if (ok) referenced[a] = referenced[b] = referenced[c] = 1;
        const int lead = __shfl(r, 0, 64);
        const bool same = ok && r == lead;
        const int k = wave_sum(same ? 1 : 0);
        if (lead != cur) {
            if (lane == 0 && cur >= 0) atomicAdd(face_count + cur, run);
            cur = lead;
            run = 0;
        }
        run += k;
        if (ok && !same) atomicAdd(face_count + r, 1);
    }
    if (lane == 0 && cur >= 0) atomicAdd(face_count + cur, run);
}

// Each wave takes MC_CHUNK consecutive vertices and folds the keys of lane 0's label as above; every lane also folds the keys
// of its referenced vertices into the box of all of them, one atomic per key per wave at the end.
__global__ __launch_bounds__(MC_BLOCK) void mc_vertex_stats_kernel(const float* __restrict__ vertices, long long n, const int* __restrict__ label,
                                                                   const int* __restrict__ referenced, unsigned* __restrict__ keys,
                                                                   unsigned* __restrict__ global_keys) {
    const int lane = threadIdx.x & 63;
    const long base = ((long)blockIdx.x * (MC_BLOCK / 64) + (threadIdx.x >> 6)) * MC_CHUNK;
    int cur = -1;
    unsigned rlo[3] = {UINT_MAX, UINT_MAX, UINT_MAX}, rhi[3] = {0u, 0u, 0u};
    unsigned glo[3] = {UINT_MAX, UINT_MAX, UINT_MAX}, ghi[3] = {0u, 0u, 0u};
    for (int step = 0; step < MC_CHUNK / 64; ++step) {
        const long v = base + step * 64 + lane;
        if (base + step * 64 >= n) break;   // wave-uniform
        const bool ok = v < n;
        const int r = ok ? label[v] : -1;
        unsigned k[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) k[d] = ok ? dsm_key(vertices[3 * v + d]) : 0u;
        if (ok && referenced[v]) {
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                glo[d] = min(glo[d], k[d]);
                ghi[d] = max(ghi[d], k[d]);
            }
        }
        const int lead = __shfl(r, 0, 64);
        const bool same = ok && r == lead;
        unsigned wlo[3], whi[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            wlo[d] = wave_min(same ? k[d] : UINT_MAX);
            whi[d] = wave_max(same ? k[d] : 0u);
        }
        if (lead != cur) {
            if (lane == 0 && cur >= 0)
#pragma unroll
                for (int d = 0; d < 3; ++d) {
                    atomicMin(keys + 6l * cur + d, rlo[d]);
                    atomicMax(keys + 6l * cur + 3 + d, rhi[d]);
                }
            cur = lead;
#pragma unroll
            for (int d = 0; d < 3; ++d) rlo[d] = UINT_MAX, rhi[d] = 0u;
        }
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            rlo[d] = min(rlo[d], wlo[d]);
            rhi[d] = max(rhi[d], whi[d]);
        }
        if (ok && !same)
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                atomicMin(keys + 6l * r + d, k[d]);
                atomicMax(keys + 6l * r + 3 + d, k[d]);
            }
    }
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        glo[d] = wave_min(glo[d]);
        ghi[d] = wave_max(ghi[d]);
    }
    if (lane == 0) {
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            if (cur >= 0) {
                atomicMin(keys + 6l * cur + d, rlo[d]);
                atomicMax(keys + 6l * cur + 3 + d, rhi[d]);
            }
            if (glo[d] != UINT_MAX) {
                atomicMin(global_keys + d, glo[d]);
                atomicMax(global_keys + 3 + d, ghi[d]);
            }
        }
    }
}

// minimum keys UINT_MAX, maximum keys 0 (no vertex yet), counts and flags 0; thread n: the global keys
__global__ __launch_bounds__(MC_BLOCK) void mc_stats_init_kernel(long long n, int* __restrict__ face_count, int* __restrict__ referenced,
                                                                 unsigned* __restrict__ keys, unsigned* __restrict__ global_keys) {
    const long v = (long)blockIdx.x * MC_BLOCK + threadIdx.x;
    if (v > n) return;
    unsigned* k = v == n ? global_keys : keys + 6 * v;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        k[d] = UINT_MAX;
        k[3 + d] = 0u;
    }
    if (v < n) {
        face_count[v] = 0;
        referenced[v] = 0;
    }
}

// The box diagonal in fp64 from the fp32 box: sqrt((dx dx + dy dy) + dz dz), dx = hi - lo in fp64.
__device__ __forceinline__ double mc_diag(const float* box) {
    const double dx = (double)box[3] - (double)box[0], dy = (double)box[4] - (double)box[1], dz = (double)box[5] - (double)box[2];
    return sqrt(dx * dx + dy * dy + dz * dz);
}

// Boxes and diagonals of every label (NaN where no vertex has it); thread n: the box of the referenced vertices.
__global__ __launch_bounds__(MC_BLOCK) void mc_stats_finalize_kernel(const unsigned* __restrict__ keys, const unsigned* __restrict__ global_keys,
                                                                     long long n, float* __restrict__ box, double* __restrict__ diag,
                                                                     float* __restrict__ global_box, double* __restrict__ global_diag) {
    const long v = (long)blockIdx.x * MC_BLOCK + threadIdx.x;
    if (v > n) return;
    const unsigned* k = v == n ? global_keys : keys + 6 * v;
    float b[6];
#pragma unroll
    for (int d = 0; d < 6; ++d) b[d] = dsm_unkey(k[d]);
    float* out = v == n ? global_box : box + 6 * v;
#pragma unroll
    for (int d = 0; d < 6; ++d) out[d] = b[d];
    if (v == n) {
        *global_diag = mc_diag(b);
    } else {
        diag[v] = mc_diag(b);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// filter
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MC_BLOCK) void mc_keep_kernel(const int* __restrict__ faces, long m, long long n, const int* __restrict__ label,
                                                           const int* __restrict__ face_count, const double* __restrict__ diag,
                                                           const double* __restrict__ global_diag, long long min_faces, double spurious,
                                                           int* __restrict__ keep) {
    const long f = (long)blockIdx.x * MC_BLOCK + threadIdx.x;
    if (f >= m) return;
    int a, b, c;
    bool k = geom_face<false>(faces, f, n, &a, &b, &c);
    if (k) {
        const int r = label[a];
        if (min_faces > 0 && (long long)face_count[r] < min_faces) k = false;
        if (spurious > 0.0 && diag[r] < *global_diag / spurious) k = false;
    }
    keep[f] = k ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------------------------------------
// smoothing
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MC_BLOCK) void mc_smooth_kernel(const float* __restrict__ in, long long n, const long long* __restrict__ offset,
                                                             const int* __restrict__ nbr, const unsigned char* __restrict__ fixed, float lambda,
                                                             float* __restrict__ out) {
    const long v = (long)blockIdx.x * MC_BLOCK + threadIdx.x;
    if (v >= n) return;
    float x = in[3 * v], y = in[3 * v + 1], z = in[3 * v + 2];
    if (!fixed[v]) {
        const long o0 = offset[v], o1 = offset[v + 1];
        float sx = 0.0f, sy = 0.0f, sz = 0.0f;
        for (long k = o0; k < o1; ++k) {
            const long u = nbr[k];
            sx += in[3 * u];
            sy += in[3 * u + 1];
            sz += in[3 * u + 2];
        }
        const float c = (float)(o1 - o0);
        x = x + lambda * (sx / c - x);
        y = y + lambda * (sy / c - y);
        z = z + lambda * (sz / c - z);
    }
    out[3 * v] = x;
    out[3 * v + 1] = y;
    out[3 * v + 2] = z;
}

// scratch layouts
struct McAdjScratch {
    size_t cnt, start, ucnt, uoff, ent, list, n_long, total, scan, bytes;
};

static McAdjScratch mc_adj_layout(long long n, long long m) {
    const size_t nv = (size_t)(n > 0 ? n : 1), ne = (size_t)(6 * m > 0 ? 6 * m : 1);
    ScratchLayout L;
    McAdjScratch s;
    s.cnt = L.take(nv * 4);
    s.start = L.take(nv * 4);
    s.ucnt = L.take(nv * 4);
    s.uoff = L.take(nv * 4);
    s.ent = L.take(ne * 4);
    s.list = L.take(nv * 4);
    s.n_long = L.take(8);
    s.total = L.take(8);
    s.scan = L.take(geom_scan_bytes(n));
    s.bytes = L.bytes;
    return s;
}

struct McStatsScratch {
    size_t keys, global_keys, referenced, bytes;
};

static McStatsScratch mc_stats_layout(long long n) {
    const size_t nv = (size_t)(n > 0 ? n : 1);
    ScratchLayout L;
    McStatsScratch s;
    s.keys = L.take(nv * 24);
    s.global_keys = L.take(24);
    s.referenced = L.take(nv * 4);
    s.bytes = L.bytes;
    return s;
}

static bool mc_sizes_ok(long long n, long long m) { return n >= 0 && n < (1ll << 31) && m >= 0 && 6 * m <= MC_MAX_ENTRIES; }

}  // namespace d3d

using namespace d3d;

#define MC_CHECK_SIZES()                                                                                                  \
    D3D_REQUIRE(mc_sizes_ok(n_vertices, n_faces), "n_vertices=%lld, n_faces=%lld (0 .. 2^31 - 1 vertices, 6 n_faces < 2^31)", \
                n_vertices, n_faces)

#define MC_CHECK_SCRATCH(need)                                                                                            \
    D3D_REQUIRE(scratch_bytes >= (need), "scratch of %zu bytes, %zu needed", scratch_bytes, (size_t)(need))

extern "C" size_t d3d_mesh_adjacency_scratch_bytes(long long n_vertices, long long n_faces) {
    if (!mc_sizes_ok(n_vertices, n_faces)) return 0;
    return mc_adj_layout(n_vertices, n_faces).bytes;
}

extern "C" int d3d_mesh_adjacency(const int* faces, long long n_faces, long long n_vertices, void* scratch, size_t scratch_bytes,
                                  long long* offset, int* nbr, unsigned char* fixed, d3d_stream_t stream) {
    D3D_REQUIRE((faces || n_faces == 0) && scratch && offset && nbr && fixed, "null pointer (faces, scratch, offset, nbr, fixed)");
    MC_CHECK_SIZES();
    const McAdjScratch L = mc_adj_layout(n_vertices, n_faces);
    MC_CHECK_SCRATCH(L.bytes);
    hipStream_t st = (hipStream_t)stream;
    char* w = (char*)scratch;
    int *cnt = (int*)(w + L.cnt), *start = (int*)(w + L.start), *ucnt = (int*)(w + L.ucnt), *uoff = (int*)(w + L.uoff);
    int *ent = (int*)(w + L.ent), *list = (int*)(w + L.list), *n_long = (int*)(w + L.n_long);
    long long* total = (long long*)(w + L.total);
    const long long n = n_vertices, m = n_faces;
    int rc = hip_status(hipMemsetAsync(cnt, 0, (size_t)(n > 0 ? n : 1) * 4, st), "mesh adjacency: clear counts");
    if (rc != D3D_OK) return rc;
    rc = hip_status(hipMemsetAsync(n_long, 0, 4, st), "mesh adjacency: clear list");
    if (rc != D3D_OK) return rc;
    if (m > 0) {
        hipLaunchKernelGGL(mc_count_kernel, dim3(ceil_div(m, MC_BLOCK)), dim3(MC_BLOCK), 0, st, faces, (long)m, n, cnt);
        D3D_LAUNCH_CHECK("mc_count_kernel launch");
    }
    rc = geom_scan(cnt, start, n, w + L.scan, total, st);   // the total is at most 6 n_faces < 2^31
    if (rc != D3D_OK) return rc;
    rc = hip_status(hipMemsetAsync(ucnt, 0, (size_t)(n > 0 ? n : 1) * 4, st), "mesh adjacency: clear fill");
    if (rc != D3D_OK) return rc;
    if (m > 0) {
        hipLaunchKernelGGL(mc_scatter_kernel, dim3(ceil_div(m, MC_BLOCK)), dim3(MC_BLOCK), 0, st, faces, (long)m, n, start, ucnt, ent);
        D3D_LAUNCH_CHECK("mc_scatter_kernel launch");
    }
    if (n > 0) {
        hipLaunchKernelGGL(mc_rows_kernel, dim3(ceil_div(n, MC_BLOCK)), dim3(MC_BLOCK), 0, st, start, cnt, n, ent, ucnt, fixed, list, n_long);
        D3D_LAUNCH_CHECK("mc_rows_kernel launch");
        hipLaunchKernelGGL(mc_rows_slow_kernel, dim3(MC_SLOW_GRID), dim3(MC_BLOCK), 0, st, start, cnt, list, n_long, ent, nbr, ucnt, fixed);
        D3D_LAUNCH_CHECK("mc_rows_slow_kernel launch");
    }
    rc = geom_scan(ucnt, uoff, n, w + L.scan, total, st);
    if (rc != D3D_OK) return rc;
    hipLaunchKernelGGL(mc_csr_kernel, dim3(ceil_div(n + 1, MC_BLOCK)), dim3(MC_BLOCK), 0, st, start, ucnt, uoff, total, n, ent, offset, nbr);
    D3D_LAUNCH_CHECK("mc_csr_kernel launch");
    return D3D_OK;
}

extern "C" int d3d_mesh_components(const int* faces, long long n_faces, long long n_vertices, int* label, int* flag, int* rounds,
                                   d3d_stream_t stream) {
    D3D_REQUIRE((faces || n_faces == 0) && label && flag, "null pointer (faces, label, flag)");
    MC_CHECK_SIZES();
    hipStream_t st = (hipStream_t)stream;
    const long long n = n_vertices, m = n_faces;
    int rc = geom_iota(label, n, st);
    if (rc != D3D_OK) return rc;
    int r = 0;
    while (m > 0 && n > 0) {
        rc = hip_status(hipMemsetAsync(flag, 0, 4, st), "mesh components: clear flag");
        if (rc != D3D_OK) return rc;
        hipLaunchKernelGGL(mc_hook_kernel, dim3(ceil_div(m, MC_BLOCK)), dim3(MC_BLOCK), 0, st, faces, (long)m, n, label, flag);
        D3D_LAUNCH_CHECK("mc_hook_kernel launch");
        ++r;
        int h = 0;
        rc = hip_status(hipMemcpyAsync(&h, flag, 4, hipMemcpyDeviceToHost, st), "mesh components: read flag");
        if (rc != D3D_OK) return rc;
        rc = hip_status(hipStreamSynchronize(st), "mesh components: sync");
        if (rc != D3D_OK) return rc;
        if (!h) break;
        rc = geom_jump(label, n, st);
        if (rc != D3D_OK) return rc;
    }
    if (rounds) *rounds = r;
    return D3D_OK;
}

extern "C" size_t d3d_mesh_stats_scratch_bytes(long long n_vertices) {
    if (!mc_sizes_ok(n_vertices, 0)) return 0;
    return mc_stats_layout(n_vertices).bytes;
}

extern "C" int d3d_mesh_component_stats(const float* vertices, long long n_vertices, const int* faces, long long n_faces, const int* label,
                                        void* scratch, size_t scratch_bytes, int* face_count, float* box, double* diag, float* global_box,
                                        double* global_diag, d3d_stream_t stream) {
    D3D_REQUIRE((vertices || n_vertices == 0) && (faces || n_faces == 0) && label && scratch && face_count && box && diag && global_box && global_diag,
                "null pointer (vertices, faces, label, scratch, face_count, box, diag, global_box, global_diag)");
    MC_CHECK_SIZES();
    const McStatsScratch L = mc_stats_layout(n_vertices);
    MC_CHECK_SCRATCH(L.bytes);
    hipStream_t st = (hipStream_t)stream;
    char* w = (char*)scratch;
    unsigned *keys = (unsigned*)(w + L.keys), *gkeys = (unsigned*)(w + L.global_keys);
    int* referenced = (int*)(w + L.referenced);
    const long long n = n_vertices, m = n_faces;
    hipLaunchKernelGGL(mc_stats_init_kernel, dim3(ceil_div(n + 1, MC_BLOCK)), dim3(MC_BLOCK), 0, st, n, face_count, referenced, keys, gkeys);
    D3D_LAUNCH_CHECK("mc_stats_init_kernel launch");
    const long long waves_f = (m + MC_CHUNK - 1) / MC_CHUNK, waves_v = (n + MC_CHUNK - 1) / MC_CHUNK;
    if (m > 0) {
        hipLaunchKernelGGL(mc_face_stats_kernel, dim3(ceil_div(waves_f, MC_BLOCK / 64)), dim3(MC_BLOCK), 0, st, faces, (long)m, n, label,
                           face_count, referenced);
        D3D_LAUNCH_CHECK("mc_face_stats_kernel launch");
    }
    if (n > 0) {
        hipLaunchKernelGGL(mc_vertex_stats_kernel, dim3(ceil_div(waves_v, MC_BLOCK / 64)), dim3(MC_BLOCK), 0, st, vertices, n, label, referenced,
                           keys, gkeys);
        D3D_LAUNCH_CHECK("mc_vertex_stats_kernel launch");
    }
    hipLaunchKernelGGL(mc_stats_finalize_kernel, dim3(ceil_div(n + 1, MC_BLOCK)), dim3(MC_BLOCK), 0, st, keys, gkeys, n, box, diag, global_box,
                       global_diag);
    D3D_LAUNCH_CHECK("mc_stats_finalize_kernel launch");
    return D3D_OK;
}

extern "C" size_t d3d_mesh_filter_scratch_bytes(long long n_faces) {
    if (!mc_sizes_ok(0, n_faces)) return 0;
    return geom_keep_layout(n_faces).bytes;
}

extern "C" int d3d_mesh_filter(const int* faces, long long n_faces, long long n_vertices, const int* label, const int* face_count,
                               const double* diag, const double* global_diag, long long min_faces, double spurious, void* scratch,
                               size_t scratch_bytes, int* out_faces, int* referenced, long long* n_kept, d3d_stream_t stream) {
    D3D_REQUIRE((faces || n_faces == 0) && label && face_count && diag && global_diag && scratch && out_faces && referenced && n_kept,
                "null pointer (faces, label, face_count, diag, global_diag, scratch, out_faces, referenced, n_kept)");
    MC_CHECK_SIZES();
    D3D_REQUIRE(min_faces >= 0, "min_faces=%lld must be >= 0", min_faces);
    D3D_REQUIRE(std::isfinite(spurious) && spurious >= 0.0, "spurious=%g must be finite and >= 0", spurious);
    const KeepScratch L = geom_keep_layout(n_faces);
    MC_CHECK_SCRATCH(L.bytes);
    hipStream_t st = (hipStream_t)stream;
    char* w = (char*)scratch;
    int* keep = (int*)(w + L.keep);
    const long long n = n_vertices, m = n_faces;
    const int rc = hip_status(hipMemsetAsync(referenced, 0, (size_t)(n > 0 ? n : 1) * 4, st), "mesh filter: clear flags");
    if (rc != D3D_OK) return rc;
    if (m > 0) {
        hipLaunchKernelGGL(mc_keep_kernel, dim3(ceil_div(m, MC_BLOCK)), dim3(MC_BLOCK), 0, st, faces, (long)m, n, label, face_count, diag,
                           global_diag, min_faces, spurious, keep);
        D3D_LAUNCH_CHECK("mc_keep_kernel launch");
    }
    return geom_scatter_kept(faces, m, nullptr, scratch, L, out_faces, referenced, n_kept, st);
}

extern "C" int d3d_mesh_smooth(const float* vertices, long long n_vertices, const long long* offset, const int* nbr, const unsigned char* fixed,
                               float lambda, int iterations, float* work, float* out, d3d_stream_t stream) {
    D3D_REQUIRE(vertices && offset && nbr && fixed && work && out, "null pointer (vertices, offset, nbr, fixed, work, out)");
    D3D_REQUIRE(n_vertices >= 0 && n_vertices < (1ll << 31), "n_vertices=%lld (0 .. 2^31 - 1)", n_vertices);
    D3D_REQUIRE(lambda > 0.0f && lambda <= 1.0f, "lambda=%g must be in (0, 1]", (double)lambda);
    D3D_REQUIRE(iterations >= 0, "iterations=%d must be >= 0", iterations);
    D3D_REQUIRE(vertices != out && vertices != work && work != out, "vertices, work and out must be distinct buffers");
    hipStream_t st = (hipStream_t)stream;
    const long long n = n_vertices;
    if (n == 0) return D3D_OK;
    if (iterations == 0)
        return hip_status(hipMemcpyAsync(out, vertices, (size_t)n * 12, hipMemcpyDeviceToDevice, st), "mesh smooth: copy");
    const float* src = vertices;
    float* dst = (iterations & 1) ? out : work;   // the last iteration writes out
    for (int it = 0; it < iterations; ++it) {
        hipLaunchKernelGGL(mc_smooth_kernel, dim3(ceil_div(n, MC_BLOCK)), dim3(MC_BLOCK), 0, st, src, n, offset, nbr, fixed, lambda, dst);
        D3D_LAUNCH_CHECK("mc_smooth_kernel launch");
        src = dst;
        dst = dst == out ? work : out;
    }
    return D3D_OK;
}
