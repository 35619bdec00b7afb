// d3h_meshdist_dev.h -- the per-triangle arithmetic of the distance-to-mesh queries, shared by the brute-force kernels of mesh_ops.hip and the BVH
// queries of bvhdist.hip: a leaf of the tree costs, and rounds, exactly what one iteration of the brute-force loop does.
//   tri_dist2        squared distance of a point to a triangle (closest point by Ericson's region test)
//   tri_closest_bary the barycentric coordinates of that closest point (same regions, same order of tests)
//   vos_term         numerator, denominator and the length product of van Oosterom-Strackee's solid-angle formula, float32
//   wsdf_angle_f64   the same solid angle in float64, for a triangle whose plane the query lies in to within rounding
#pragma once
#include "d3h_vec.h"

namespace {

__device__ __forceinline__ float tri_dist2(V3 p, V3 a, V3 ab, V3 ac) {
    V3 ap = p - a;
    float d1 = dot(ab, ap), d2 = dot(ac, ap);
    if (d1 <= 0.f && d2 <= 0.f) return dot(ap, ap);                                   // vertex a
    V3 bp = ap - ab;
    float d3 = dot(ab, bp), d4 = dot(ac, bp);
    if (d3 >= 0.f && d4 <= d3) return dot(bp, bp);                                     // vertex b
    float vc = d1 * d4 - d3 * d2;
    if (vc <= 0.f && d1 >= 0.f && d3 <= 0.f) { V3 q = ap - ab * (d1 / (d1 - d3)); return dot(q, q); }      // edge ab
    V3 cp = ap - ac;
    float d5 = dot(ab, cp), d6 = dot(ac, cp);
    if (d6 >= 0.f && d5 <= d6) return dot(cp, cp);                                     // vertex c
    float vb = d5 * d2 - d1 * d6;
    if (vb <= 0.f && d2 >= 0.f && d6 <= 0.f) { V3 q = ap - ac * (d2 / (d2 - d6)); return dot(q, q); }      // edge ac
    float va = d3 * d6 - d5 * d4;
    if (va <= 0.f && (d4 - d3) >= 0.f && (d5 - d6) >= 0.f) {                           // edge bc
        float w = (d4 - d3) / ((d4 - d3) + (d5 - d6));
        V3 q = bp - (ac - ab) * w;
        return dot(q, q);
    }
    float denom = 1.0f / (va + vb + vc);                                               // interior
    V3 q = ap - ab * (vb * denom) - ac * (vc * denom);
    return dot(q, q);
}

// weights (of a, b, c) of the point tri_dist2 measures to; each >= 0, their sum 1 to within two roundings
__device__ __forceinline__ V3 tri_closest_bary(V3 p, V3 a, V3 ab, V3 ac) {
    V3 ap = p - a;
    float d1 = dot(ab, ap), d2 = dot(ac, ap);
    if (d1 <= 0.f && d2 <= 0.f) return mk(1.f, 0.f, 0.f);
    V3 bp = ap - ab;
    float d3 = dot(ab, bp), d4 = dot(ac, bp);
    if (d3 >= 0.f && d4 <= d3) return mk(0.f, 1.f, 0.f);
    float vc = d1 * d4 - d3 * d2;
    if (vc <= 0.f && d1 >= 0.f && d3 <= 0.f) { float t = fminf(d1 / (d1 - d3), 1.f); return mk(1.f - t, t, 0.f); }
    V3 cp = ap - ac;
    float d5 = dot(ab, cp), d6 = dot(ac, cp);
    if (d6 >= 0.f && d5 <= d6) return mk(0.f, 0.f, 1.f);
    float vb = d5 * d2 - d1 * d6;
    if (vb <= 0.f && d2 >= 0.f && d6 <= 0.f) { float t = fminf(d2 / (d2 - d6), 1.f); return mk(1.f - t, 0.f, t); }
    float va = d3 * d6 - d5 * d4;
    if (va <= 0.f && (d4 - d3) >= 0.f && (d5 - d6) >= 0.f) {
        float t = fminf((d4 - d3) / ((d4 - d3) + (d5 - d6)), 1.f);
        return mk(0.f, 1.f - t, t);
    }
    float denom = 1.0f / (va + vb + vc);
    float v = fminf(fmaxf(vb * denom, 0.f), 1.f), w = fminf(fmaxf(vc * denom, 0.f), 1.f - v);
    return mk(1.f - v - w, v, w);
}

// solid angle of the triangle (a, a + ab, a + ac) seen from p = 2 atan2(det, den); lll = |ra| |rb| |rc|, the scale det is judged against
struct VosTerm { float det, den, lll; };
__device__ __forceinline__ VosTerm vos_term(V3 p, V3 a, V3 ab, V3 ac) {
    V3 ra = a - p, rb = ra + ab, rc = ra + ac;
    float la = sqrtf(dot(ra, ra)), lb = sqrtf(dot(rb, rb)), lc = sqrtf(dot(rc, rc));
    VosTerm t;
    t.det = dot(ra, cross(rb, rc));
    t.den = la * lb * lc + dot(ra, rb) * lc + dot(ra, rc) * lb + dot(rb, rc) * la;
    t.lll = la * lb * lc;
    return t;
}

// 2 atan2(det, den) of van Oosterom-Strackee for one triangle, in float64 from the float32 vertices q0, q1, q2
__device__ float wsdf_angle_f64(V3 p, const float* __restrict__ q0, const float* __restrict__ q1, const float* __restrict__ q2) {
    double r[3][3], l[3];
    for (int k = 0; k < 3; ++k) {
        const float* q = k == 0 ? q0 : (k == 1 ? q1 : q2);
        r[k][0] = (double)q[0] - (double)p.x, r[k][1] = (double)q[1] - (double)p.y, r[k][2] = (double)q[2] - (double)p.z;
        l[k] = sqrt(r[k][0] * r[k][0] + r[k][1] * r[k][1] + r[k][2] * r[k][2]);
    }
    const double cx = r[1][1] * r[2][2] - r[1][2] * r[2][1], cy = r[1][2] * r[2][0] - r[1][0] * r[2][2], cz = r[1][0] * r[2][1] - r[1][1] * r[2][0];
    const double det = r[0][0] * cx + r[0][1] * cy + r[0][2] * cz;
    const double d01 = r[0][0] * r[1][0] + r[0][1] * r[1][1] + r[0][2] * r[1][2], d02 = r[0][0] * r[2][0] + r[0][1] * r[2][1] + r[0][2] * r[2][2];
    const double d12 = r[1][0] * r[2][0] + r[1][1] * r[2][1] + r[1][2] * r[2][2];
    return (float)(2.0 * atan2(det, l[0] * l[1] * l[2] + d01 * l[2] + d02 * l[1] + d12 * l[0]));
}
__device__ __forceinline__ float wsdf_angle_f64(V3 p, const float* __restrict__ v, const int* __restrict__ ff) {
    return wsdf_angle_f64(p, v + 3 * (size_t)ff[0], v + 3 * (size_t)ff[1], v + 3 * (size_t)ff[2]);
}

}  // namespace
