// Surface mesh from the depth maps: the semantics are this project's (deep3d_aerial_amd/mesh.py states them,
// include/deep3d_planesweep.h too).  The reference builds its mesh with OpenMVS binaries, which this project does not run.
//
// mark:      one lane per pixel; the back-projected pixel centre's brick gets a byte flag in a grid padded by one brick.
//            Idempotent stores, no atomics.
// bricks:    the 3^3 dilation of the flags per brick, the shared scan (geom_shared.h), then the brick list and the dense index grid.
// integrate: one workgroup per allocated brick, one lane per voxel.  Every wave tests 64 views at a time against the brick's
//            box (8 corners, one ballot) and walks the set bits in increasing view order; sums stay in registers, one store per
//            voxel per call.
// count:     per voxel the 8 corners of its cube (through the index grid where they leave the brick), the crossed owned edges
//            and the triangles of its 6 tetrahedra; two scans give the output offsets.
// emit:      the same corners again; vertices at the owned edges, triangles through the owners' offsets.
// compact:   scan of the referenced flags, scatter of the kept vertices, renumbering of the triangles.
// Every store has one writer (or writers of the same value); every sum has a fixed order.
#include <cmath>
#include <cstdint>

#include "common.h"
#include "geom_shared.h"

namespace d3d {

constexpr int MESH_BRICK = 512;   // 8^3 voxels, one lane each
static_assert(sizeof(d3d_mesh_view_t) == 192, "d3d_mesh_view_t: the layout deep3d_aerial_amd/mesh.py fills");

// The 6 Kuhn tetrahedra of a cube around its diagonal 0 -> 7 (corner c = x | y << 1 | z << 2), one per axis permutation in
// lexicographic order, each listed with positive orientation; the 6 edges of a tetrahedron are (0,1) (0,2) (0,3) (1,2) (1,3) (2,3)
// of that list.  MESH_TRI[case] (bit i of case: corner i inside) holds up to 2 triangles as edge numbers, oriented so that the
// right-hand normal points from the inside to the outside; mesh.py has the same tables and tests/test_mesh.py derives them.
constexpr int MESH_TET[6][4] = {{0, 1, 3, 7}, {0, 5, 1, 7}, {0, 3, 2, 7}, {0, 2, 6, 7}, {0, 4, 5, 7}, {0, 6, 4, 7}};
__constant__ int MESH_EDGE[6][2] = {{0, 1}, {0, 2}, {0, 3}, {1, 2}, {1, 3}, {2, 3}};
__constant__ int MESH_NTRI[16] = {0, 1, 1, 2, 1, 2, 2, 1, 1, 2, 2, 1, 2, 1, 1, 0};
__constant__ int MESH_TRI[16][2][3] = {
    {{0, 0, 0}, {0, 0, 0}}, {{0, 1, 2}, {0, 0, 0}}, {{0, 4, 3}, {0, 0, 0}}, {{1, 2, 4}, {1, 4, 3}},
    {{1, 3, 5}, {0, 0, 0}}, {{0, 5, 2}, {0, 3, 5}}, {{0, 4, 5}, {0, 5, 1}}, {{2, 4, 5}, {0, 0, 0}},
    {{2, 5, 4}, {0, 0, 0}}, {{0, 1, 5}, {0, 5, 4}}, {{0, 5, 3}, {0, 2, 5}}, {{1, 5, 3}, {0, 0, 0}},
    {{1, 3, 4}, {1, 4, 2}}, {{0, 3, 4}, {0, 0, 0}}, {{0, 2, 1}, {0, 0, 0}}, {{0, 0, 0}, {0, 0, 0}}};
// (MESH_TET and MESH_TYPE_CORNER are only read in unrolled loops: the corner numbers fold to constants and the cube's register
// arrays are never indexed at run time, which would put them in scratch)
// owned edge types in output order: the corner at the far end of +x, +y, +z, +xy, +xz, +yz, +xyz; and back
constexpr int MESH_TYPE_CORNER[7] = {1, 2, 4, 3, 5, 6, 7};
__constant__ int MESH_TYPE_OF[8] = {-1, 0, 1, 3, 2, 4, 5, 6};

__device__ __forceinline__ double mesh_coord(double lo, double s, int i) { return lo + ((double)i + 0.5) * s; }

// linear brick index of padded / unpadded grids
__device__ __forceinline__ long mesh_pad_index(const d3d_mesh_grid_t& g, int bi, int bj, int bk) {
    return ((long)(bk + 1) * (g.by + 2) + (bj + 1)) * (g.bx + 2) + (bi + 1);
}

// ---------------------------------------------------------------------------------------------------------------------------
// allocation
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mesh_mark_kernel(d3d_mesh_grid_t g, const d3d_mesh_view_t* __restrict__ views, double thr,
                                                        unsigned char* __restrict__ marks) {
    const d3d_mesh_view_t& V = views[blockIdx.y];
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= (long)V.W * V.H) return;
    const float D = V.depth[p], c = V.conf[p];
    if (!(isfinite(D) && D > 0.0f && (double)c >= thr)) return;
    const int y = (int)(p / V.W), x = (int)(p - (long)y * V.W);
    const double d = (double)D;
    const double yn = ((double)y - V.K[5]) / V.K[4];
    const double xn = ((double)x - V.K[2] - V.K[1] * yn) / V.K[0];
    const double c0 = xn * d - V.t[0], c1 = yn * d - V.t[1], c2 = d - V.t[2];
    const double X[3] = {V.R[0] * c0 + V.R[3] * c1 + V.R[6] * c2, V.R[1] * c0 + V.R[4] * c1 + V.R[7] * c2,
                         V.R[2] * c0 + V.R[5] * c1 + V.R[8] * c2};
    const double lo[3] = {g.x_min, g.y_min, g.z_min};
    const int nb[3] = {g.bx, g.by, g.bz};
    int b[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double fb = floor(floor((X[a] - lo[a]) / g.voxel) / 8.0);
        if (!(fb >= -1.0 && fb <= (double)nb[a])) return;   // NaN too
        b[a] = (int)fb;
    }
    marks[mesh_pad_index(g, b[0], b[1], b[2])] = 1;
}

__device__ __forceinline__ bool mesh_dilated(const d3d_mesh_grid_t& g, const unsigned char* marks, long b) {
    const int bi = (int)(b % g.bx), bj = (int)((b / g.bx) % g.by), bk = (int)(b / ((long)g.bx * g.by));
    bool any = false;
    for (int dk = -1; dk <= 1; ++dk)
        for (int dj = -1; dj <= 1; ++dj)
            for (int di = -1; di <= 1; ++di) any |= marks[mesh_pad_index(g, bi + di, bj + dj, bk + dk)] != 0;
    return any;
}

__global__ __launch_bounds__(256) void mesh_dilate_kernel(d3d_mesh_grid_t g, const unsigned char* __restrict__ marks, long n,
                                                          int* __restrict__ flag) {
    const long b = (long)blockIdx.x * 256 + threadIdx.x;
    if (b < n) flag[b] = mesh_dilated(g, marks, b) ? 1 : 0;
}

__global__ __launch_bounds__(256) void mesh_list_kernel(d3d_mesh_grid_t g, const unsigned char* __restrict__ marks, long n,
                                                        int* __restrict__ brick_index, int* __restrict__ brick_list) {
    const long b = (long)blockIdx.x * 256 + threadIdx.x;
    if (b >= n) return;
    const int off = brick_index[b];
    if (mesh_dilated(g, marks, b)) {
        brick_list[off] = (int)b;
    } else {
        brick_index[b] = -1;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// integration
// ---------------------------------------------------------------------------------------------------------------------------
// May view V observe a voxel centre in the box [lo, hi]?  False only when all 8 corners lie in front of the view and their
// projections' bounding box misses the image by more than a pixel (a projective map keeps convexity where q2 > 0).
__device__ __forceinline__ bool mesh_box_visible(const d3d_mesh_view_t& V, const double* lo, const double* hi) {
    double umin = INFINITY, umax = -INFINITY, vmin = INFINITY, vmax = -INFINITY;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const GeomPq r = geom_project(V, (k & 1) ? hi[0] : lo[0], (k & 2) ? hi[1] : lo[1], (k & 4) ? hi[2] : lo[2]);
        if (!(r.p2 > 0.0 && r.q2 > 0.0)) return true;
        const double u = r.q0 / r.q2, v = r.q1 / r.q2;
        if (!(isfinite(u) && isfinite(v))) return true;
        umin = fmin(umin, u);
        umax = fmax(umax, u);
        vmin = fmin(vmin, v);
        vmax = fmax(vmax, v);
    }
    return !(umax < -1.0 || umin > (double)V.W || vmax < -1.0 || vmin > (double)V.H);
}

__global__ __launch_bounds__(MESH_BRICK) void mesh_integrate_kernel(d3d_mesh_grid_t g, const int* __restrict__ brick_list,
                                                                    const d3d_mesh_view_t* __restrict__ views, int n_views, double trunc,
                                                                    double thr, float* __restrict__ sum, int* __restrict__ count) {
    const int b = brick_list[blockIdx.x];
    const int bi = b % g.bx, bj = (b / g.bx) % g.by, bk = b / (g.bx * g.by);
    const int lx = threadIdx.x & 7, ly = (threadIdx.x >> 3) & 7, lz = threadIdx.x >> 6;
    const int gi = bi * 8 + lx, gj = bj * 8 + ly, gk = bk * 8 + lz;
    const bool exists = gi < g.nx && gj < g.ny && gk < g.nz;
    const double X0 = mesh_coord(g.x_min, g.voxel, gi), X1 = mesh_coord(g.y_min, g.voxel, gj), X2 = mesh_coord(g.z_min, g.voxel, gk);
    // the box of the brick's existing voxel centres (wave-uniform)
    const double lo[3] = {mesh_coord(g.x_min, g.voxel, bi * 8), mesh_coord(g.y_min, g.voxel, bj * 8), mesh_coord(g.z_min, g.voxel, bk * 8)};
    const double hi[3] = {mesh_coord(g.x_min, g.voxel, min(bi * 8 + 7, g.nx - 1)), mesh_coord(g.y_min, g.voxel, min(bj * 8 + 7, g.ny - 1)),
                          mesh_coord(g.z_min, g.voxel, min(bk * 8 + 7, g.nz - 1))};
    const long slot = (long)blockIdx.x * MESH_BRICK + threadIdx.x;
    float s = exists ? sum[slot] : 0.0f;
    int n = exists ? count[slot] : 0;
    const int lane = threadIdx.x & 63;
    for (int w = 0; w * 64 < n_views; ++w) {
        const int vl = w * 64 + lane;
        const bool cand = vl < n_views && mesh_box_visible(views[vl], lo, hi);
        unsigned long long bits = __ballot(cand);
        while (bits) {
            const int vi = __builtin_amdgcn_readfirstlane(w * 64 + __builtin_ctzll(bits));
            bits &= bits - 1;
            if (!exists) continue;
            const d3d_mesh_view_t& V = views[vi];
            const GeomPq r = geom_project(V, X0, X1, X2);
            if (!(r.p2 > 0.0 && r.q2 > 0.0)) continue;
            const double px = floor(r.q0 / r.q2 + 0.5), py = floor(r.q1 / r.q2 + 0.5);
            if (!(px >= 0.0 && px <= (double)(V.W - 1) && py >= 0.0 && py <= (double)(V.H - 1))) continue;
            const long pix = (long)py * V.W + (long)px;
            const float D = V.depth[pix], c = V.conf[pix];
            if (!(isfinite(D) && D > 0.0f && (double)c >= thr)) continue;
            const double sdf = (double)D - r.p2;
            if (!(sdf >= -trunc)) continue;
            s += (float)fmin(1.0, sdf / trunc);
            n += 1;
        }
    }
    if (exists) {
        sum[slot] = s;
        count[slot] = n;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// extraction
// ---------------------------------------------------------------------------------------------------------------------------
struct MeshCube {
    long slot[8];   // -1: the corner does not exist or its brick is not allocated
    float f[8];
    bool obs[8];
    int gi, gj, gk;
    bool exists;
};

__device__ __forceinline__ long mesh_slot(const d3d_mesh_grid_t& g, const int* brick_index, int gi, int gj, int gk) {
    if (gi >= g.nx || gj >= g.ny || gk >= g.nz) return -1;
    const int b = brick_index[((long)(gk >> 3) * g.by + (gj >> 3)) * g.bx + (gi >> 3)];
    if (b < 0) return -1;
    return (long)b * MESH_BRICK + (((gk & 7) * 8 + (gj & 7)) * 8 + (gi & 7));
}

__device__ __forceinline__ void mesh_load_cube(const d3d_mesh_grid_t& g, const int* __restrict__ brick_list, const int* __restrict__ brick_index,
                                               const float* __restrict__ sum, const int* __restrict__ count, int min_views, MeshCube& c) {
    const int b = brick_list[blockIdx.x];
    const int bi = b % g.bx, bj = (b / g.bx) % g.by, bk = b / (g.bx * g.by);
    c.gi = bi * 8 + (threadIdx.x & 7);
    c.gj = bj * 8 + ((threadIdx.x >> 3) & 7);
    c.gk = bk * 8 + (threadIdx.x >> 6);
    c.exists = c.gi < g.nx && c.gj < g.ny && c.gk < g.nz;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        c.slot[k] = k == 0 ? (c.exists ? (long)blockIdx.x * MESH_BRICK + threadIdx.x : -1)
                           : mesh_slot(g, brick_index, c.gi + (k & 1), c.gj + ((k >> 1) & 1), c.gk + ((k >> 2) & 1));
        const int n = c.slot[k] >= 0 ? count[c.slot[k]] : 0;
        c.obs[k] = c.slot[k] >= 0 && n >= min_views;
        c.f[k] = c.obs[k] ? sum[c.slot[k]] / (float)n : 0.0f;
    }
}

__device__ __forceinline__ int mesh_edge_mask(const MeshCube& c) {
    int m = 0;
#pragma unroll
    for (int t = 0; t < 7; ++t) {
        const int k = MESH_TYPE_CORNER[t];
        if (c.obs[0] && c.obs[k] && ((c.f[0] < 0.0f) != (c.f[k] < 0.0f))) m |= 1 << t;
    }
    return m;
}

__device__ __forceinline__ int mesh_tet_case(const MeshCube& c, int t) {
    int m = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int k = MESH_TET[t][i];
        if (!c.obs[k]) return -1;
        if (c.f[k] < 0.0f) m |= 1 << i;
    }
    return m;
}

__global__ __launch_bounds__(MESH_BRICK) void mesh_count_kernel(d3d_mesh_grid_t g, const int* __restrict__ brick_list,
                                                                const int* __restrict__ brick_index, const float* __restrict__ sum,
                                                                const int* __restrict__ count, int min_views, unsigned char* __restrict__ edges,
                                                                int* __restrict__ n_verts, int* __restrict__ n_faces) {
    MeshCube c;
    mesh_load_cube(g, brick_list, brick_index, sum, count, min_views, c);
    int m = 0, nf = 0;
    if (c.exists) {
        m = mesh_edge_mask(c);
#pragma unroll
        for (int t = 0; t < 6; ++t) {
            const int cs = mesh_tet_case(c, t);
            if (cs >= 0) nf += MESH_NTRI[cs];
        }
    }
    const long slot = (long)blockIdx.x * MESH_BRICK + threadIdx.x;
    edges[slot] = (unsigned char)m;
    n_verts[slot] = __popc(m);
    n_faces[slot] = nf;
}

__global__ __launch_bounds__(MESH_BRICK) void mesh_emit_kernel(d3d_mesh_grid_t g, const int* __restrict__ brick_list,
                                                               const int* __restrict__ brick_index, const float* __restrict__ sum,
                                                               const int* __restrict__ count, int min_views,
                                                               const unsigned char* __restrict__ edges, const int* __restrict__ vert_base,
                                                               const int* __restrict__ face_base, float* __restrict__ vertices,
                                                               int* __restrict__ faces, int* __restrict__ referenced) {
    MeshCube c;
    mesh_load_cube(g, brick_list, brick_index, sum, count, min_views, c);
    if (!c.exists) return;
    const long slot = c.slot[0];
    const int m = edges[slot];
    int vid = vert_base[slot];
#pragma unroll
    for (int t = 0; t < 7; ++t) {
        if (!((m >> t) & 1)) continue;
        const int k = MESH_TYPE_CORNER[t];
        const double fa = (double)c.f[0], fb = (double)c.f[k];
        const double w = fa / (fa - fb);
        const int ga[3] = {c.gi, c.gj, c.gk};
        const double lo[3] = {g.x_min, g.y_min, g.z_min};
        for (int a = 0; a < 3; ++a) {
            const double xa = mesh_coord(lo[a], g.voxel, ga[a]), xb = mesh_coord(lo[a], g.voxel, ga[a] + ((k >> a) & 1));
            vertices[(long)vid * 3 + a] = (float)(xa + w * (xb - xa));
        }
        ++vid;
    }
    int fid = face_base[slot];
#pragma unroll
    for (int t = 0; t < 6; ++t) {
        const int cs = mesh_tet_case(c, t);
        if (cs < 0) continue;
        const int tc[4] = {MESH_TET[t][0], MESH_TET[t][1], MESH_TET[t][2], MESH_TET[t][3]};
        for (int q = 0; q < MESH_NTRI[cs]; ++q) {
            for (int e = 0; e < 3; ++e) {
                const int le = MESH_TRI[cs][q][e], ea = MESH_EDGE[le][0], eb = MESH_EDGE[le][1];
                const int ca = ea == 0 ? tc[0] : ea == 1 ? tc[1] : ea == 2 ? tc[2] : tc[3];
                const int cb = eb == 0 ? tc[0] : eb == 1 ? tc[1] : eb == 2 ? tc[2] : tc[3];
                const int lo = __popc(ca) < __popc(cb) ? ca : cb, hi = ca ^ cb ^ lo;
                const int type = MESH_TYPE_OF[hi ^ lo];
                // the owner is a corner of a meshed tetrahedron: observed, so it has a slot
                const long owner = lo == 0 ? slot : mesh_slot(g, brick_index, c.gi + (lo & 1), c.gj + ((lo >> 1) & 1), c.gk + ((lo >> 2) & 1));
                const int v = vert_base[owner] + __popc(edges[owner] & ((1 << type) - 1));
                faces[(long)fid * 3 + e] = v;
                referenced[v] = 1;
            }
            ++fid;
        }
    }
}

__global__ __launch_bounds__(256) void mesh_scatter_kernel(const float* __restrict__ vertices, long n, const int* __restrict__ referenced,
                                                           const int* __restrict__ remap, float* __restrict__ out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n || !referenced[i]) return;
    const long o = remap[i];
    out[o * 3] = vertices[i * 3];
    out[o * 3 + 1] = vertices[i * 3 + 1];
    out[o * 3 + 2] = vertices[i * 3 + 2];
}

__global__ __launch_bounds__(256) void mesh_renumber_kernel(int* __restrict__ faces, long n, const int* __restrict__ remap) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) faces[i] = remap[faces[i]];
}

static const char* mesh_grid_error(const d3d_mesh_grid_t* g) {
    if (!g) return "null grid";
    if (!(std::isfinite(g->x_min) && std::isfinite(g->y_min) && std::isfinite(g->z_min))) return "grid minimum not finite";
    if (!(std::isfinite(g->voxel) && g->voxel > 0.0)) return "voxel size must be finite and > 0";
    if (g->nx < 1 || g->ny < 1 || g->nz < 1) return "grid size must be >= 1 per axis";
    if (g->bx != ceil_div(g->nx, 8) || g->by != ceil_div(g->ny, 8) || g->bz != ceil_div(g->nz, 8)) return "bricks per axis must be ceil(n / 8)";
    if ((long long)(g->bx + 2) * (g->by + 2) * (g->bz + 2) >= (1ll << 31)) return "brick count does not fit in int32";
    return nullptr;
}

static bool mesh_views_ok(int n_views) { return n_views >= 0 && n_views < (1 << 20); }

}  // namespace d3d

using namespace d3d;

#define MESH_CHECK_GRID()                                  \
    do {                                                   \
        const char* _e = mesh_grid_error(grid);            \
        D3D_REQUIRE(_e == nullptr, "mesh grid: %s", _e);   \
    } while (0)

extern "C" int d3d_mesh_mark(const d3d_mesh_grid_t* grid, const d3d_mesh_view_t* views, int n_views, int max_pixels, double conf_threshold,
                             unsigned char* marks, d3d_stream_t stream) {
    D3D_REQUIRE(grid && marks, "null pointer (grid, marks)");
    MESH_CHECK_GRID();
    D3D_REQUIRE(mesh_views_ok(n_views), "n_views=%d (0 .. 2^20 - 1)", n_views);
    D3D_REQUIRE(views || n_views == 0, "null pointer (views) with %d views", n_views);
    D3D_REQUIRE(max_pixels >= 0, "max_pixels=%d must be >= 0", max_pixels);
    D3D_REQUIRE(!std::isnan(conf_threshold), "conf_threshold is NaN");
    if (n_views == 0 || max_pixels == 0) return D3D_OK;
    hipLaunchKernelGGL(mesh_mark_kernel, dim3(ceil_div(max_pixels, 256), n_views), dim3(256), 0, (hipStream_t)stream, *grid, views,
                       conf_threshold, marks);
    D3D_LAUNCH_CHECK("mesh_mark_kernel launch");
    return D3D_OK;
}

extern "C" int d3d_mesh_bricks(const d3d_mesh_grid_t* grid, const unsigned char* marks, void* scratch, size_t scratch_bytes, int* brick_index,
                               int* brick_list, long long* n_bricks, d3d_stream_t stream) {
    D3D_REQUIRE(grid && marks && scratch && brick_index && brick_list && n_bricks,
                "null pointer (grid, marks, scratch, brick_index, brick_list, n_bricks)");
    MESH_CHECK_GRID();
    const long long n = (long long)grid->bx * grid->by * grid->bz;
    D3D_REQUIRE(scratch_bytes >= d3d_mesh_scan_scratch_bytes(n), "scratch of %zu bytes, %zu needed (d3d_mesh_scan_scratch_bytes)",
                scratch_bytes, d3d_mesh_scan_scratch_bytes(n));
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(mesh_dilate_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, st, *grid, marks, (long)n, brick_index);
    D3D_LAUNCH_CHECK("mesh_dilate_kernel launch");
    const int rc = geom_scan(brick_index, brick_index, n, scratch, n_bricks, st);
    if (rc != D3D_OK) return rc;
    hipLaunchKernelGGL(mesh_list_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, st, *grid, marks, (long)n, brick_index, brick_list);
    D3D_LAUNCH_CHECK("mesh_list_kernel launch");
    return D3D_OK;
}

#define MESH_CHECK_BRICKS()                                                                                                     \
    D3D_REQUIRE(n_bricks >= 0 && (long long)n_bricks <= (long long)grid->bx * grid->by * grid->bz &&                            \
                    (long long)n_bricks * MESH_BRICK < (1ll << 31),                                                            \
                "n_bricks=%d (0 .. the grid's bricks, n_bricks * 512 < 2^31)", n_bricks)

extern "C" int d3d_mesh_integrate(const d3d_mesh_grid_t* grid, const int* brick_list, int n_bricks, const d3d_mesh_view_t* views, int n_views,
                                  double trunc, double conf_threshold, float* sum, int* count, d3d_stream_t stream) {
    D3D_REQUIRE(grid && brick_list && sum && count, "null pointer (grid, brick_list, sum, count)");
    MESH_CHECK_GRID();
    MESH_CHECK_BRICKS();
    D3D_REQUIRE(mesh_views_ok(n_views), "n_views=%d (0 .. 2^20 - 1)", n_views);
    D3D_REQUIRE(views || n_views == 0, "null pointer (views) with %d views", n_views);
    D3D_REQUIRE(std::isfinite(trunc) && trunc > 0.0 && trunc <= 8.0 * grid->voxel, "trunc=%g must be in (0, 8 voxel]", trunc);
    D3D_REQUIRE(!std::isnan(conf_threshold), "conf_threshold is NaN");
    if (n_views == 0 || n_bricks == 0) return D3D_OK;
    hipLaunchKernelGGL(mesh_integrate_kernel, dim3(n_bricks), dim3(MESH_BRICK), 0, (hipStream_t)stream, *grid, brick_list, views, n_views,
                       trunc, conf_threshold, sum, count);
    D3D_LAUNCH_CHECK("mesh_integrate_kernel launch");
    return D3D_OK;
}

extern "C" int d3d_mesh_count(const d3d_mesh_grid_t* grid, const int* brick_list, const int* brick_index, int n_bricks, const float* sum,
                              const int* count, int min_views, void* scratch, size_t scratch_bytes, unsigned char* edges, int* vert_base,
                              int* face_base, long long* totals, d3d_stream_t stream) {
    D3D_REQUIRE(grid && brick_list && brick_index && sum && count && scratch && edges && vert_base && face_base && totals,
                "null pointer (grid, brick_list, brick_index, sum, count, scratch, edges, vert_base, face_base, totals)");
    MESH_CHECK_GRID();
    MESH_CHECK_BRICKS();
    D3D_REQUIRE(min_views >= 1, "min_views=%d must be >= 1", min_views);
    const long long n = (long long)n_bricks * MESH_BRICK;
    D3D_REQUIRE(scratch_bytes >= d3d_mesh_scan_scratch_bytes(n), "scratch of %zu bytes, %zu needed (d3d_mesh_scan_scratch_bytes)",
                scratch_bytes, d3d_mesh_scan_scratch_bytes(n));
    hipStream_t st = (hipStream_t)stream;
    if (n_bricks > 0) {
        hipLaunchKernelGGL(mesh_count_kernel, dim3(n_bricks), dim3(MESH_BRICK), 0, st, *grid, brick_list, brick_index, sum, count, min_views,
                           edges, vert_base, face_base);
        D3D_LAUNCH_CHECK("mesh_count_kernel launch");
    }
    int rc = geom_scan(vert_base, vert_base, n, scratch, totals, st);
    if (rc != D3D_OK) return rc;
    return geom_scan(face_base, face_base, n, scratch, totals + 1, st);
}

extern "C" int d3d_mesh_emit(const d3d_mesh_grid_t* grid, const int* brick_list, const int* brick_index, int n_bricks, const float* sum,
                             const int* count, int min_views, const unsigned char* edges, const int* vert_base, const int* face_base,
                             float* vertices, int* faces, int* referenced, d3d_stream_t stream) {
    D3D_REQUIRE(grid && brick_list && brick_index && sum && count && edges && vert_base && face_base && vertices && faces && referenced,
                "null pointer (grid, brick_list, brick_index, sum, count, edges, vert_base, face_base, vertices, faces, referenced)");
    MESH_CHECK_GRID();
    MESH_CHECK_BRICKS();
    D3D_REQUIRE(min_views >= 1, "min_views=%d must be >= 1", min_views);
    if (n_bricks == 0) return D3D_OK;
    hipLaunchKernelGGL(mesh_emit_kernel, dim3(n_bricks), dim3(MESH_BRICK), 0, (hipStream_t)stream, *grid, brick_list, brick_index, sum, count,
                       min_views, edges, vert_base, face_base, vertices, faces, referenced);
    D3D_LAUNCH_CHECK("mesh_emit_kernel launch");
    return D3D_OK;
}

extern "C" int d3d_mesh_compact(const float* vertices, long long n_vertices, int* faces, long long n_faces, const int* referenced, void* scratch,
                                size_t scratch_bytes, int* remap, float* out_vertices, long long* n_kept, d3d_stream_t stream) {
    D3D_REQUIRE(vertices && faces && referenced && scratch && remap && out_vertices && n_kept,
                "null pointer (vertices, faces, referenced, scratch, remap, out_vertices, n_kept)");
    D3D_REQUIRE(n_vertices >= 0 && n_vertices < (1ll << 31) && n_faces >= 0 && n_faces < (1ll << 31),
                "n_vertices=%lld, n_faces=%lld (0 .. 2^31 - 1)", n_vertices, n_faces);
    D3D_REQUIRE(scratch_bytes >= d3d_mesh_scan_scratch_bytes(n_vertices), "scratch of %zu bytes, %zu needed (d3d_mesh_scan_scratch_bytes)",
                scratch_bytes, d3d_mesh_scan_scratch_bytes(n_vertices));
    hipStream_t st = (hipStream_t)stream;
    const int rc = geom_scan(referenced, remap, n_vertices, scratch, n_kept, st);
    if (rc != D3D_OK) return rc;
    if (n_vertices > 0) {
        hipLaunchKernelGGL(mesh_scatter_kernel, dim3(ceil_div(n_vertices, 256)), dim3(256), 0, st, vertices, (long)n_vertices, referenced, remap,
                           out_vertices);
        D3D_LAUNCH_CHECK("mesh_scatter_kernel launch");
    }
    if (n_faces > 0) {
        hipLaunchKernelGGL(mesh_renumber_kernel, dim3(ceil_div(n_faces * 3, 256)), dim3(256), 0, st, faces, (long)(n_faces * 3), remap);
        D3D_LAUNCH_CHECK("mesh_renumber_kernel launch");
    }
    return D3D_OK;
}
