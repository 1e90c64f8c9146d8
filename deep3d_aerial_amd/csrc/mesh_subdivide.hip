// Subdividing the surface mesh where the images outresolve it: every edge whose projection is longer than
// max_edge pixels in some view that sees both its ends gets its midpoint, and every face is replaced by the conforming split of
// its marked edges.  The rule is this project's (deep3d_aerial_amd/subdivide.py states it, include/deep3d_planesweep.h too); it
// does not claim to match OpenMVS's RefineMesh subdivision.
//
// measure: one lane per edge of the lexicographic unique-edge list (d3d_mesh_decimate_edges), looping over the call's views (a
//          view's record is the same address in every lane, as in rf_views_kernel).  Both endpoints and the running maximum stay
//          in registers; both endpoints pass the frustum test before either depth map is touched.  The list is sorted by its
//          first index, so neighbouring lanes share or neighbour an endpoint.  The lane max-merges into measure[e]: it owns it.
// plan:    one lane per edge: the fp32 midpoint and the mark; a scan of the marks ranks the split edges.  One lane per face: the
//          three edge indices by a binary search of (min, max) in the edge list, the child count 1 + (marked edges); a scan of
//          the counts places the children.  A one-lane kernel copies the two totals.
// emit:    the input vertices come through first (one copy); one lane per edge writes the midpoint of a split edge at
//          n_vertices + rank; one lane per face writes its children from its offset on.
// The candidate test is ortho's, from geom_shared.h: geom_uv, then geom_depth_at under the same comparison.
// No atomics at all; every float result is a fixed-order fp64 computation without contraction, so nothing depends on the order
// the lanes run in, and a maximum does not depend on view order, batching or rank split.
#include <climits>
#include <cmath>
#include <cstdint>

#include "common.h"
#include "geom_shared.h"

namespace d3d {

constexpr int MS_BLOCK = 256;

// The edges the passes read: *n_edges clamped to 0 .. max_edges (the list holds no more).
__device__ __forceinline__ long long ms_edge_count(const long long* __restrict__ n_edges, long long max_edges) {
    const long long ne = *n_edges;
    return ne < 0 ? 0 : (ne > max_edges ? max_edges : ne);
}

// ---------------------------------------------------------------------------------------------------------------------------
// measure
// ---------------------------------------------------------------------------------------------------------------------------
// The depth test at the pixel of (u, v), which geom_uv has placed inside the image.
__device__ __forceinline__ bool ms_unhidden(const d3d_mesh_view_t& V, double u, double v, double p2, double tol1) {
    const float D = geom_depth_at(V, u, v);
    return isfinite(D) && D > 0.0f && p2 <= (double)D * tol1;
}

__global__ __launch_bounds__(MS_BLOCK) void ms_measure_kernel(const float* __restrict__ vertices, long long n, const int* __restrict__ edges,
                                                              const long long* __restrict__ n_edges, long long max_edges,
                                                              const d3d_mesh_view_t* __restrict__ views, int n_views, double tol1,
                                                              double* __restrict__ measure) {
    const long e = (long)blockIdx.x * MS_BLOCK + threadIdx.x;
    if (e >= ms_edge_count(n_edges, max_edges)) return;
    const int a = edges[2 * e], b = edges[2 * e + 1];
    if (a < 0 || a >= n || b < 0 || b >= n) return;   // not this mesh's list
    double XA[3], XB[3];
    geom_load3(vertices, a, XA);
    geom_load3(vertices, b, XB);
    double best = measure[e];
    for (int vi = 0; vi < n_views; ++vi) {
        const d3d_mesh_view_t& V = views[vi];
        if (!V.depth || V.W < 1 || V.H < 1) continue;
        double ua, va, pa, ub, vb, pb;
        if (!geom_uv(V, XA[0], XA[1], XA[2], &ua, &va, &pa)) continue;
        if (!geom_uv(V, XB[0], XB[1], XB[2], &ub, &vb, &pb)) continue;
        if (!ms_unhidden(V, ua, va, pa, tol1)) continue;
        if (!ms_unhidden(V, ub, vb, pb, tol1)) continue;
        const double du = ua - ub, dv = va - vb;
        const double l2 = du * du + dv * dv;
        if (!isfinite(l2)) continue;
        best = l2 > best ? l2 : best;
    }
    measure[e] = best;
}

// ---------------------------------------------------------------------------------------------------------------------------
// plan
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MS_BLOCK) void ms_mark_kernel(const float* __restrict__ vertices, long long n, const int* __restrict__ edges,
                                                           const long long* __restrict__ n_edges, long long max_edges,
                                                           const double* __restrict__ measure, double max_edge2, int* __restrict__ mark,
                                                           float* __restrict__ midpoint) {
    const long e = (long)blockIdx.x * MS_BLOCK + threadIdx.x;
    if (e >= max_edges) return;
    float mid[3] = {0.0f, 0.0f, 0.0f};
    bool split = false;
    if (e < ms_edge_count(n_edges, max_edges)) {
        const int a = edges[2 * e], b = edges[2 * e + 1];
        if (a >= 0 && a < n && b >= 0 && b < n) {
            bool from_a = false, from_b = false;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float xa = vertices[3l * a + c], xb = vertices[3l * b + c];
                mid[c] = (float)(((double)xa + (double)xb) * 0.5);
                from_a = from_a || mid[c] != xa;
                from_b = from_b || mid[c] != xb;
            }
            split = measure[e] > max_edge2 && from_a && from_b;
        }
    }
    mark[e] = split ? 1 : 0;
    midpoint[3 * e] = mid[0];
    midpoint[3 * e + 1] = mid[1];
    midpoint[3 * e + 2] = mid[2];
}

// The index of edge {x, y} in the list (lexicographic (a, b), a < b), or -1.
__device__ __forceinline__ int ms_find(const int* __restrict__ edges, long long ne, int x, int y) {
    const int a = min(x, y), b = max(x, y);
    long long lo = 0, hi = ne;   // the first entry >= (a, b) lies in lo .. hi
    while (lo < hi) {
        const long long mid = lo + (hi - lo) / 2;
        const int ea = edges[2 * mid], eb = edges[2 * mid + 1];
        if (ea < a || (ea == a && eb < b))
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo < ne && edges[2 * lo] == a && edges[2 * lo + 1] == b ? (int)lo : -1;
}

__global__ __launch_bounds__(MS_BLOCK) void ms_faces_kernel(const int* __restrict__ faces, long m, long long n, const int* __restrict__ edges,
                                                            const long long* __restrict__ n_edges, long long max_edges,
                                                            const int* __restrict__ mark, int* __restrict__ face_edge,
                                                            int* __restrict__ child_count) {
    const long f = (long)blockIdx.x * MS_BLOCK + threadIdx.x;
    if (f >= m) return;
    int v0, v1, v2, e0 = -1, e1 = -1, e2 = -1, count = 1;
    if (geom_face<true>(faces, f, n, &v0, &v1, &v2)) {
        const long long ne = ms_edge_count(n_edges, max_edges);
        e0 = ms_find(edges, ne, v0, v1);
        e1 = ms_find(edges, ne, v1, v2);
        e2 = ms_find(edges, ne, v2, v0);
        if (e0 >= 0 && e1 >= 0 && e2 >= 0)
            count += (mark[e0] ? 1 : 0) + (mark[e1] ? 1 : 0) + (mark[e2] ? 1 : 0);
        else
            e0 = e1 = e2 = -1;   // a face whose edges the list does not hold comes through as it is
    }
    face_edge[3 * f] = e0;
    face_edge[3 * f + 1] = e1;
    face_edge[3 * f + 2] = e2;
    child_count[f] = count;
}

// totals[0] = the split edges, totals[1] = the faces after the split
__global__ void ms_totals_kernel(const long long* __restrict__ splits, const long long* __restrict__ faces_out, long long* __restrict__ totals) {
    totals[0] = *splits;
    totals[1] = *faces_out;
}

// ---------------------------------------------------------------------------------------------------------------------------
// emit
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MS_BLOCK) void ms_emit_vertices_kernel(long long n, const long long* __restrict__ n_edges, long long max_edges,
                                                                    const int* __restrict__ mark, const int* __restrict__ rank,
                                                                    const float* __restrict__ midpoint, long long n_split,
                                                                    float* __restrict__ out_vertices) {
    const long e = (long)blockIdx.x * MS_BLOCK + threadIdx.x;
    if (e >= ms_edge_count(n_edges, max_edges) || !mark[e]) return;
    const long long r = rank[e];
    if (r < 0 || r >= n_split) return;   // not this plan's ranks
    float* x = out_vertices + 3 * (n + r);
    x[0] = midpoint[3 * e];
    x[1] = midpoint[3 * e + 1];
    x[2] = midpoint[3 * e + 2];
}

__device__ __forceinline__ void ms_put(int* __restrict__ out_faces, long long g, int a, int b, int c) {
    out_faces[3 * g] = a;
    out_faces[3 * g + 1] = b;
    out_faces[3 * g + 2] = c;
}

// |x - y|^2 = (dx^2 + dy^2) + dz^2 in fp64 on fp32 positions
__device__ __forceinline__ double ms_dist2(const float* __restrict__ x, const float* __restrict__ y) {
    const double dx = (double)x[0] - (double)y[0], dy = (double)x[1] - (double)y[1], dz = (double)x[2] - (double)y[2];
    return (dx * dx + dy * dy) + dz * dz;
}

__global__ __launch_bounds__(MS_BLOCK) void ms_emit_faces_kernel(const float* __restrict__ vertices, long long n, const int* __restrict__ faces,
                                                                 long m, long long max_edges, const int* __restrict__ mark,
                                                                 const int* __restrict__ rank, const float* __restrict__ midpoint,
                                                                 const int* __restrict__ face_edge, const int* __restrict__ child_offset,
                                                                 long long n_split, long long n_faces_out, int* __restrict__ out_faces) {
    const long f = (long)blockIdx.x * MS_BLOCK + threadIdx.x;
    if (f >= m) return;
    const int v[3] = {faces[3 * f], faces[3 * f + 1], faces[3 * f + 2]};
    const int fe[3] = {face_edge[3 * f], face_edge[3 * f + 1], face_edge[3 * f + 2]};
    int mid[3] = {-1, -1, -1};   // the midpoint's vertex index of a split edge
    bool ok = fe[0] >= 0 && fe[0] < max_edges && fe[1] >= 0 && fe[1] < max_edges && fe[2] >= 0 && fe[2] < max_edges;
    int split = 0;
    if (ok) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            if (!mark[fe[i]]) continue;
            const long long r = rank[fe[i]];
            ok = ok && r >= 0 && r < n_split;   // anything else is not this plan's data
            mid[i] = (int)(n + r);
            ++split;
        }
    }
    if (!ok) split = 0;
    const long long g = child_offset[f];
    if (g < 0 || g + split + 1 > n_faces_out) return;   // not this plan's offsets
    if (split == 0) {
        ms_put(out_faces, g, v[0], v[1], v[2]);
    } else if (split == 1) {
        const int i = mid[0] >= 0 ? 0 : (mid[1] >= 0 ? 1 : 2);
        const int a = v[i], b = v[(i + 1) % 3], c = v[(i + 2) % 3], mi = mid[i];
        ms_put(out_faces, g, a, mi, c);
        ms_put(out_faces, g + 1, mi, b, c);
    } else if (split == 2) {
        const int i = mid[0] < 0 ? 0 : (mid[1] < 0 ? 1 : 2);   // the unsplit edge
        const int j = (i + 1) % 3, k = (i + 2) % 3;
        const int a = v[i], b = v[j], c = v[k], p = mid[j], q = mid[k];
        ms_put(out_faces, g, p, c, q);
        bool through_a = a < b;   // a tie: the diagonal that starts at the smaller of a and b
        if (a >= 0 && a < n && b >= 0 && b < n) {
            const double ap = ms_dist2(vertices + 3l * a, midpoint + 3l * fe[j]), bq = ms_dist2(vertices + 3l * b, midpoint + 3l * fe[k]);
            if (ap < bq) through_a = true;
            if (bq < ap) through_a = false;
        }
        if (through_a) {
            ms_put(out_faces, g + 1, a, b, p);
            ms_put(out_faces, g + 2, a, p, q);
        } else {
            ms_put(out_faces, g + 1, a, b, q);
            ms_put(out_faces, g + 2, b, p, q);
        }
    } else {
        ms_put(out_faces, g, v[0], mid[0], mid[2]);
        ms_put(out_faces, g + 1, mid[0], v[1], mid[1]);
        ms_put(out_faces, g + 2, mid[2], mid[1], v[2]);
        ms_put(out_faces, g + 3, mid[0], mid[1], mid[2]);
    }
}

// scratch of the plan
struct MsPlanScratch {
    size_t splits, faces_out, scan, bytes;
};

static MsPlanScratch ms_plan_layout(long long m, long long max_edges) {
    ScratchLayout L;
    MsPlanScratch s;
    s.splits = L.take(8);
    s.faces_out = L.take(8);
    s.scan = L.take(geom_scan_bytes(m > max_edges ? m : max_edges));
    s.bytes = L.bytes;
    return s;
}

static bool ms_sizes_ok(long long n, long long m, long long max_edges) {
    return n >= 0 && n < (1ll << 31) && m >= 0 && 6 * m < (1ll << 31) && max_edges >= 0 && max_edges < (1ll << 31);
}

}  // namespace d3d

using namespace d3d;

#define MS_CHECK_SIZES()                                                                                                          \
    D3D_REQUIRE(ms_sizes_ok(n_vertices, n_faces, max_edges),                                                                      \
                "n_vertices=%lld, n_faces=%lld, max_edges=%lld (0 .. 2^31 - 1 vertices and edges, 6 n_faces < 2^31)", n_vertices, \
                n_faces, max_edges)

extern "C" int d3d_mesh_subdivide_measure(const float* vertices, long long n_vertices, const int* edges, const long long* n_edges,
                                          long long max_edges, const d3d_mesh_view_t* views, int n_views, double depth_tolerance,
                                          double* measure, d3d_stream_t stream) {
    D3D_REQUIRE((vertices || n_vertices == 0) && edges && n_edges && (views || n_views == 0) && measure,
                "null pointer (vertices, edges, n_edges, views, measure)");
    const long long n_faces = 0;
    MS_CHECK_SIZES();
    D3D_REQUIRE(n_views >= 0 && n_views < (1 << 20), "n_views=%d (0 .. 2^20 - 1)", n_views);
    D3D_REQUIRE(std::isfinite(depth_tolerance) && depth_tolerance >= 0.0, "depth_tolerance=%g must be finite and >= 0", depth_tolerance);
    if (max_edges == 0 || n_views == 0 || n_vertices == 0) return D3D_OK;
    hipLaunchKernelGGL(ms_measure_kernel, dim3(ceil_div(max_edges, MS_BLOCK)), dim3(MS_BLOCK), 0, (hipStream_t)stream, vertices, n_vertices, edges,
                       n_edges, max_edges, views, n_views, 1.0 + depth_tolerance, measure);
    D3D_LAUNCH_CHECK("ms_measure_kernel launch");
    return D3D_OK;
}

extern "C" size_t d3d_mesh_subdivide_scratch_bytes(long long n_faces, long long max_edges) {
    if (!ms_sizes_ok(0, n_faces, max_edges)) return 0;
    return ms_plan_layout(n_faces, max_edges).bytes;
}

extern "C" int d3d_mesh_subdivide_plan(const float* vertices, long long n_vertices, const int* faces, long long n_faces, const int* edges,
                                       const long long* n_edges, long long max_edges, const double* measure, double max_edge, void* scratch,
                                       size_t scratch_bytes, int* mark, int* rank, float* midpoint, int* face_edge, int* child_count,
                                       int* child_offset, long long* totals, d3d_stream_t stream) {
    D3D_REQUIRE((vertices || n_vertices == 0) && (faces || n_faces == 0) && edges && n_edges && measure && scratch && mark && rank && midpoint &&
                    face_edge && child_count && child_offset && totals,
                "null pointer (vertices, faces, edges, n_edges, measure, scratch, mark, rank, midpoint, face_edge, child_count, "
                "child_offset, totals)");
    MS_CHECK_SIZES();
    D3D_REQUIRE(std::isfinite(max_edge) && max_edge >= 1.0, "max_edge=%g must be a finite pixel length >= 1", max_edge);
    const MsPlanScratch L = ms_plan_layout(n_faces, max_edges);
    D3D_REQUIRE(scratch_bytes >= L.bytes, "scratch of %zu bytes, %zu needed", scratch_bytes, L.bytes);
    hipStream_t st = (hipStream_t)stream;
    char* w = (char*)scratch;
    long long *splits = (long long*)(w + L.splits), *faces_out = (long long*)(w + L.faces_out);
    const long long n = n_vertices, m = n_faces;
    if (max_edges > 0) {
        hipLaunchKernelGGL(ms_mark_kernel, dim3(ceil_div(max_edges, MS_BLOCK)), dim3(MS_BLOCK), 0, st, vertices, n, edges, n_edges, max_edges,
                           measure, max_edge * max_edge, mark, midpoint);
        D3D_LAUNCH_CHECK("ms_mark_kernel launch");
    }
    int rc = geom_scan(mark, rank, max_edges, w + L.scan, splits, st);   // at most max_edges < 2^31
    if (rc != D3D_OK) return rc;
    if (m > 0) {
        hipLaunchKernelGGL(ms_faces_kernel, dim3(ceil_div(m, MS_BLOCK)), dim3(MS_BLOCK), 0, st, faces, (long)m, n, edges, n_edges, max_edges, mark,
                           face_edge, child_count);
        D3D_LAUNCH_CHECK("ms_faces_kernel launch");
    }
    rc = geom_scan(child_count, child_offset, m, w + L.scan, faces_out, st);   // at most 4 n_faces < 2^31
    if (rc != D3D_OK) return rc;
    hipLaunchKernelGGL(ms_totals_kernel, dim3(1), dim3(1), 0, st, splits, faces_out, totals);
    D3D_LAUNCH_CHECK("ms_totals_kernel launch");
    return D3D_OK;
}

extern "C" int d3d_mesh_subdivide_emit(const float* vertices, long long n_vertices, const int* faces, long long n_faces, const long long* n_edges,
                                       long long max_edges, const int* mark, const int* rank, const float* midpoint, const int* face_edge,
                                       const int* child_offset, long long n_split, long long n_faces_out, float* out_vertices, int* out_faces,
                                       d3d_stream_t stream) {
    D3D_REQUIRE((vertices || n_vertices == 0) && (faces || n_faces == 0) && n_edges && mark && rank && midpoint && face_edge && child_offset &&
                    out_vertices && out_faces,
                "null pointer (vertices, faces, n_edges, mark, rank, midpoint, face_edge, child_offset, out_vertices, out_faces)");
    MS_CHECK_SIZES();
    D3D_REQUIRE(n_split >= 0 && n_split <= max_edges && n_vertices + n_split < (1ll << 31) && n_faces_out >= n_faces &&
                    n_faces_out <= 4 * n_faces && 6 * n_faces_out < (1ll << 31),
                "n_split=%lld, n_faces_out=%lld (0 .. max_edges splits, n_vertices + n_split < 2^31, n_faces .. 4 n_faces faces, "
                "6 n_faces_out < 2^31)",
                n_split, n_faces_out);
    D3D_REQUIRE(vertices != out_vertices && faces != out_faces, "the outputs must not be the inputs");
    hipStream_t st = (hipStream_t)stream;
    const long long n = n_vertices, m = n_faces;
    int rc = D3D_OK;
    if (n > 0) rc = hip_status(hipMemcpyAsync(out_vertices, vertices, (size_t)n * 12, hipMemcpyDeviceToDevice, st), "mesh subdivide emit: copy vertices");
    if (rc != D3D_OK) return rc;
    if (max_edges > 0 && n_split > 0) {
        hipLaunchKernelGGL(ms_emit_vertices_kernel, dim3(ceil_div(max_edges, MS_BLOCK)), dim3(MS_BLOCK), 0, st, n, n_edges, max_edges, mark, rank,
                           midpoint, n_split, out_vertices);
        D3D_LAUNCH_CHECK("ms_emit_vertices_kernel launch");
    }
    if (m > 0) {
        hipLaunchKernelGGL(ms_emit_faces_kernel, dim3(ceil_div(m, MS_BLOCK)), dim3(MS_BLOCK), 0, st, vertices, n, faces, (long)m, max_edges, mark, rank,
                           midpoint, face_edge, child_offset, n_split, n_faces_out, out_faces);
        D3D_LAUNCH_CHECK("ms_emit_faces_kernel launch");
    }
    return D3D_OK;
}
