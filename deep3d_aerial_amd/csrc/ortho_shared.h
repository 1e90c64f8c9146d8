// The fp64 projection ortho.hip and texture.hip share (not part of the public ABI): p = R X + t, q = K p, each row summed left to
// right, u = q0 / q2, v = q1 / q2 (built with -ffp-contract=off: no contraction).
#pragma once
#include "common.h"

namespace d3d {

struct OrthoPq {
    double p2, q0, q1, q2;
};

__device__ __forceinline__ OrthoPq ortho_project(const d3d_ortho_view_t& V, double X0, double X1, double X2) {
    const double p0 = V.R[0] * X0 + V.R[1] * X1 + V.R[2] * X2 + V.t[0];
    const double p1 = V.R[3] * X0 + V.R[4] * X1 + V.R[5] * X2 + V.t[1];
    const double p2 = V.R[6] * X0 + V.R[7] * X1 + V.R[8] * X2 + V.t[2];
    OrthoPq r;
    r.p2 = p2;
    r.q0 = V.K[0] * p0 + V.K[1] * p1 + V.K[2] * p2;
    r.q1 = V.K[3] * p0 + V.K[4] * p1 + V.K[5] * p2;
    r.q2 = V.K[6] * p0 + V.K[7] * p1 + V.K[8] * p2;
    return r;
}

// (u, v) of X in view V when it lies in front of the view and inside its image, else false.
__device__ __forceinline__ bool ortho_uv(const d3d_ortho_view_t& V, double X0, double X1, double X2, double* u, double* v, double* p2) {
    const OrthoPq r = ortho_project(V, X0, X1, X2);
    if (!(r.p2 > 0.0 && r.q2 > 0.0)) return false;
    *u = r.q0 / r.q2;
    *v = r.q1 / r.q2;
    *p2 = r.p2;
    return *u >= 0.0 && *u <= (double)(V.W - 1) && *v >= 0.0 && *v <= (double)(V.H - 1);
}

}  // namespace d3d
