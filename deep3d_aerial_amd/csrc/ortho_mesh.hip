// Orthophoto of the textured mesh (deep3d_aerial_amd/ortho_mesh.py states the rule, include/deep3d_planesweep.h
// too, tests/test_ortho_mesh.py restates it).  The mesh is seen from above (or, with z_down, from below: the side the cameras are
// on) on a DsmGrid, every cell sampling its centre; the colour comes from the texture atlas through the face's texcoords.
//
// Coverage and height are the mesh DSM's (dsm_tri.h: one copy of the set-up, the cell range, the edge functions and the sample).
// The texcoords travel with the vertices through the lexicographic sort; at a covered centre s = ((w_a s_a + w_b s_b) + w_c s_c) / W
// in fp64 (t alike), the texel position on page k = texnumber is x = s P - 0.5, y = (1 - t) h_k - 0.5 (the inverse of
// tx_texcoords_kernel), the colour geom_tap there, each channel floor(c + 0.5) clamped to 0 .. 255, alpha 255.  A face whose three
// texcoord pairs are equal bit for bit (what tx_texcoords_kernel writes for a face no view sees), whose texnumber is outside
// 0 .. n_pages - 1 or with a non-finite texcoord is untextured: it still occludes, with the colour word 0.
//
// A cell keeps the largest 64-bit key (zk << 32) | colour word, zk = dsm_key(z), or ~dsm_key(z) with z_down (the lowest sample
// wins).  No finite z has dsm_key 0 or 0xffffffff, so key 0 is the empty cell in both modes.  Equal heights (coincident faces,
// shared edges that round alike) go to the larger colour word: a textured face (alpha 255) beats an untextured one.  Every update
// is a 64-bit integer atomicMax whose result is not used: the raster is a function of the set of (triangle, texcoords, texels).
//
// small:    one lane per face, cell ranges of at most OM_SMALL cells; larger ranges go to the big list.
// big:      the persistent grid of dsm_tri_big_kernel, the same chunk ownership.
// Per covered centre (both): the height first, then a plain load of the cell's key; when the face's zk is already below the
// key's upper half the sampling is skipped.  Keys only grow, so a stale read costs a redundant sample and never a wrong one.
// finalize: key -> rgba and height.
#include <cmath>

#include "cloud_search.h"
#include "common.h"
#include "dsm_tri.h"
#include "geom_shared.h"

namespace d3d {

constexpr int OM_SMALL = 64;   // cell ranges of at most this many cells: one lane, no list (dsm.hip's DSM_TRI_SMALL)

// What a face carries besides its coverage: the texcoords of its sorted vertices and its page.
struct OmTex {
    double s[3], t[3];
    const unsigned* page;   // null: untextured
    int P, h;
};

struct OmAtlas {
    const float* texcoord;
    const int* texnumber;
    const unsigned* atlas;
    const long long* page_row;
    int n_pages, P;
};

__device__ __forceinline__ void om_face_tex(const OmAtlas& A, long f, const int (&corner)[3], OmTex& X) {
    X.page = nullptr;
    X.P = A.P;
    X.h = 0;
    float st[6];
#pragma unroll
    for (int q = 0; q < 6; ++q) st[q] = A.texcoord[6 * f + q];
    bool finite = true;
#pragma unroll
    for (int q = 0; q < 6; ++q) finite = finite && isfinite(st[q]);
    const bool same = __float_as_uint(st[0]) == __float_as_uint(st[2]) && __float_as_uint(st[2]) == __float_as_uint(st[4]) &&
                      __float_as_uint(st[1]) == __float_as_uint(st[3]) && __float_as_uint(st[3]) == __float_as_uint(st[5]);
    const int k = A.texnumber[f];
#pragma unroll
    for (int v = 0; v < 3; ++v) {
        // corner[v] is 0, 1 or 2: selects instead of a dynamic index keep st in registers
        const int c = corner[v];
        X.s[v] = (double)(c == 0 ? st[0] : (c == 1 ? st[2] : st[4]));
        X.t[v] = (double)(c == 0 ? st[1] : (c == 1 ? st[3] : st[5]));
    }
    if (!finite || same || k < 0 || k >= A.n_pages) return;
    const long long r0 = A.page_row[k], r1 = A.page_row[k + 1];
    // the Python layer refuses a page_row that is not increasing: a guard that keeps the loads inside the page_row[n_pages] rows
    if (r0 < 0 || r1 <= r0 || r1 - r0 > 0x7fffffffll || r1 > A.page_row[A.n_pages]) return;
    X.page = A.atlas + r0 * (long long)A.P;
    X.h = (int)(r1 - r0);
}

// The cell's update for a face that covers its centre with height z.
__device__ __forceinline__ void om_cell(const OmTex& X, const double (&w)[3], double W, float z, bool z_down,
                                        unsigned long long* cell) {
    const unsigned k = dsm_key(z);
    const unsigned zk = z_down ? ~k : k;
    const unsigned long long seen = *cell;   // plain load: a stale value is a smaller key
    if (zk < (unsigned)(seen >> 32)) return;
    unsigned word = 0u;
    if (X.page) {
        const double s = ((w[0] * X.s[0] + w[1] * X.s[1]) + w[2] * X.s[2]) / W;
        const double t = ((w[0] * X.t[0] + w[1] * X.t[1]) + w[2] * X.t[2]) / W;
        const double x = s * (double)X.P - 0.5, y = (1.0 - t) * (double)X.h - 0.5;
        double c[3];
        geom_tap(X.page, X.P, X.h, x, y, c);
        word = 0xff000000u;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) word |= (unsigned)fmin(fmax(floor(c[ch] + 0.5), 0.0), 255.0) << (8 * ch);
    }
    atomicMax(cell, ((unsigned long long)zk << 32) | word);
}

__global__ __launch_bounds__(DSM_BLOCK) void om_small_kernel(const float* __restrict__ vertices, int n_vertices,
                                                             const int* __restrict__ faces, int n_faces, OmAtlas A, DsmGrid g,
                                                             int z_down, unsigned long long* __restrict__ keys,
                                                             int4* __restrict__ big, int* __restrict__ n_big) {
    const long f = (long)blockIdx.x * DSM_BLOCK + threadIdx.x;
    if (f >= n_faces) return;
    DsmTri T;
    int j0, j1, i0, i1, corner[3];
    if (!dsm_tri_setup(vertices, n_vertices, faces, f, T, corner) || !dsm_tri_range(T, g, &j0, &j1, &i0, &i1)) return;
    const int nj = j1 - j0 + 1, ni = i1 - i0 + 1;
    if ((long)nj * ni > OM_SMALL) {
        const int q = atomicAdd(n_big, 1);
        if (q < n_faces) big[q] = make_int4((int)f, i0 * g.W + j0, nj, ni);   // always true (one slot per face): a guard on the write
        return;
    }
    OmTex X;
    om_face_tex(A, f, corner, X);
    for (int i = i0; i <= i1; ++i)
        for (int j = j0; j <= j1; ++j) {
            float z;
            double w[3], W;
            if (dsm_tri_sample(T, g, i, j, &z, w, &W)) om_cell(X, w, W, z, z_down != 0, keys + (long)i * g.W + j);
        }
}

__global__ __launch_bounds__(DSM_BLOCK) void om_big_kernel(const float* __restrict__ vertices, int n_vertices,
                                                           const int* __restrict__ faces, int n_faces, OmAtlas A, DsmGrid g, int z_down,
                                                           const int4* __restrict__ big, const int* __restrict__ n_big,
                                                           unsigned long long* __restrict__ keys) {
    __shared__ int4 ent[DSM_BLOCK];
    __shared__ int first[DSM_BLOCK];
    const int nb = min(*n_big, n_faces);
    const int G = gridDim.x, b = blockIdx.x, t = threadIdx.x;
    for (int base = 0; base < nb; base += DSM_BLOCK) {
        const int q = base + t;
        int k0 = -1;
        if (q < nb) {
            const int4 e = big[q];
            ent[t] = e;
            const long chunks = ((long)e.z * e.w + DSM_TRI_CHUNK - 1) / DSM_TRI_CHUNK;
            const int k = dsm_tri_first_chunk(q, b, G);
            k0 = k < chunks ? k : -1;
        }
        first[t] = k0;
        __syncthreads();
        const int m = min(DSM_BLOCK, nb - base);
        for (int e = 0; e < m; ++e) {
            const int k1 = first[e];   // uniform across the workgroup
            if (k1 < 0) continue;
            const int4 en = ent[e];
            DsmTri T;
            int corner[3];
            if (!dsm_tri_setup(vertices, n_vertices, faces, en.x, T, corner)) continue;   // listed faces passed it: a guard
            OmTex X;
            om_face_tex(A, en.x, corner, X);
            const int cells = en.z * en.w;
            const int j0 = en.y % g.W, i0 = en.y / g.W;
            for (long k = k1; k * DSM_TRI_CHUNK < cells; k += G)
                for (int u = 0; u < DSM_TRI_CHUNK; u += DSM_BLOCK) {
                    const long idx = k * DSM_TRI_CHUNK + u + t;
                    if (idx >= cells) break;
                    const int r = (int)(idx / en.z), c = (int)(idx - (long)r * en.z);
                    const int i = i0 + r, j = j0 + c;
                    float z;
                    double w[3], W;
                    if (i < g.H && j < g.W && dsm_tri_sample(T, g, i, j, &z, w, &W))
                        om_cell(X, w, W, z, z_down != 0, keys + (long)i * g.W + j);
                }
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(DSM_BLOCK) void om_finalize_kernel(const unsigned long long* __restrict__ keys, int cells, int z_down,
                                                                unsigned* __restrict__ rgba, float* __restrict__ height) {
    const int c = blockIdx.x * DSM_BLOCK + threadIdx.x;
    if (c >= cells) return;
    const unsigned long long k = keys[c];
    const unsigned zk = (unsigned)(k >> 32);
    rgba[c] = (unsigned)k;   // 0 in an empty cell and under an untextured face
    height[c] = k ? dsm_unkey(z_down ? ~zk : zk) : __builtin_nanf("");
}

struct OmScratch {
    size_t keys, n_big, big, total;
};

static OmScratch om_layout(long long n_faces, long long cells) {
    ScratchLayout L;
    OmScratch s = {};
    s.keys = L.take((size_t)cells * 8);
    s.n_big = L.take(4);
    s.big = L.take((size_t)n_faces * 16);
    s.total = L.bytes;
    return s;
}

static bool om_dims_ok(long long n, int W, int H) {
    return n >= 0 && n < (1ll << 31) && W >= 1 && H >= 1 && (long long)W * H < (1ll << 31);
}

}  // namespace d3d

using namespace d3d;

extern "C" size_t d3d_ortho_mesh_scratch_bytes(long long n_faces, int W, int H) {
    if (!om_dims_ok(n_faces, W, H)) return 0;
    return om_layout(n_faces, (long long)W * H).total;
}

extern "C" int d3d_ortho_from_mesh(const float* vertices, long long n_vertices, const int* faces, long long n_faces,
                                   const float* texcoord, const int* texnumber, const unsigned* atlas, const long long* page_row,
                                   int n_pages, int page_width, double x_min, double y_max, double unit_x, double unit_y,
                                   double z_min, double z_max, int W, int H, int z_down, void* scratch, size_t scratch_bytes,
                                   unsigned* rgba, float* height, d3d_stream_t stream) {
    D3D_REQUIRE(rgba && height && scratch, "null pointer (rgba, height, scratch)");
    D3D_REQUIRE(atlas && page_row, "null pointer (atlas, page_row)");
    D3D_REQUIRE(vertices || n_vertices == 0, "null pointer (vertices) with %lld vertices", n_vertices);
    D3D_REQUIRE((faces && texcoord && texnumber) || n_faces == 0, "null pointer (faces, texcoord, texnumber) with %lld faces", n_faces);
    D3D_REQUIRE(n_vertices >= 0 && n_vertices < (1ll << 31), "n_vertices=%lld (0 .. 2^31 - 1)", n_vertices);
    D3D_REQUIRE(n_faces >= 0 && n_faces < (1ll << 31), "n_faces=%lld (0 .. 2^31 - 1)", n_faces);
    D3D_REQUIRE(n_pages >= 1, "n_pages=%d (>= 1)", n_pages);
    D3D_REQUIRE(page_width >= 1, "page_width=%d (>= 1)", page_width);
    D3D_REQUIRE(W >= 1 && H >= 1 && (long long)W * H < (1ll << 31), "raster %d x %d: size must be >= 1 and W * H < 2^31", W, H);
    D3D_REQUIRE(std::isfinite(unit_x) && std::isfinite(unit_y) && unit_x > 0.0 && unit_y > 0.0, "unit (%g, %g) must be finite and > 0",
                unit_x, unit_y);
    D3D_REQUIRE(std::isfinite(x_min) && std::isfinite(y_max), "border (x_min %g, y_max %g) must be finite", x_min, y_max);
    D3D_REQUIRE(!std::isnan(z_min) && !std::isnan(z_max) && z_min <= z_max, "z bounds [%g, %g]", z_min, z_max);
    D3D_REQUIRE(z_down == 0 || z_down == 1, "z_down=%d (0 or 1)", z_down);
    const long long cells = (long long)W * H;
    const OmScratch L = om_layout(n_faces, cells);
    D3D_REQUIRE(scratch_bytes >= L.total, "scratch of %zu bytes, %zu needed (d3d_ortho_mesh_scratch_bytes)", scratch_bytes, L.total);
    const SearchRange R[3] = {{rgba, (size_t)cells * 4}, {height, (size_t)cells * 4}, {scratch, scratch_bytes}};
    D3D_REQUIRE(search_apart(R, 3), "rgba, height and scratch must not alias");
    // page_row is device memory: the host cannot read it here.  The kernels treat a page whose rows are not increasing as
    // untextured; ortho_mesh.mesh_to_ortho refuses such an array before the call.
    const int nf = (int)n_faces, nc = (int)cells;
    const DsmGrid g = {x_min, y_max, unit_x, unit_y, z_min, z_max, W, H};
    const OmAtlas A = {texcoord, texnumber, atlas, page_row, n_pages, page_width};
    hipStream_t st = (hipStream_t)stream;
    char* s = (char*)scratch;
    unsigned long long* keys = (unsigned long long*)(s + L.keys);
    int* n_big = (int*)(s + L.n_big);
    int4* big = (int4*)(s + L.big);
    int rc = hip_status(hipMemsetAsync(keys, 0, (size_t)cells * 8, st), "ortho mesh: clear keys");
    if (rc != D3D_OK) return rc;
    rc = hip_status(hipMemsetAsync(n_big, 0, 4, st), "ortho mesh: clear list");
    if (rc != D3D_OK) return rc;
    if (nf > 0) {
        hipLaunchKernelGGL(om_small_kernel, dim3(ceil_div(nf, DSM_BLOCK)), dim3(DSM_BLOCK), 0, st, vertices, (int)n_vertices, faces, nf, A,
                           g, z_down, keys, big, n_big);
        D3D_LAUNCH_CHECK("om_small_kernel launch");
        hipLaunchKernelGGL(om_big_kernel, dim3(DSM_TRI_GRID), dim3(DSM_BLOCK), 0, st, vertices, (int)n_vertices, faces, nf, A, g, z_down,
                           big, n_big, keys);
        D3D_LAUNCH_CHECK("om_big_kernel launch");
    }
    hipLaunchKernelGGL(om_finalize_kernel, dim3(ceil_div(nc, DSM_BLOCK)), dim3(DSM_BLOCK), 0, st, keys, nc, z_down, rgba, height);
    D3D_LAUNCH_CHECK("om_finalize_kernel launch");
    return D3D_OK;
}
