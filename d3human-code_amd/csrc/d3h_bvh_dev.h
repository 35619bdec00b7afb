// d3h_bvh_dev.h -- node layout and any-hit traversal of the triangle BVH built by bvh.hip, shared with envshade.hip (shadow rays).
//
// Nodes.  A mesh of F triangles has F - 1 internal nodes (0 .. F-2, node 0 is the root) followed by F leaves (node F-1+j holds the j-th
// triangle in Morton order); F = 1 is the single leaf 0.  A node is two float4:
//     {lo.x, lo.y, lo.z, link}   link: internal = index of the left child (>= 0); leaf = ~j (< 0), j the row of the leaf-ordered triangles
//     {hi.x, hi.y, hi.z, rope}   rope: the node to go on with when this subtree is done or missed, -1 = traversal over
// The rope of a node is the right sibling of its first ancestor-or-self that is a left child, so "descend left on a hit, follow the rope
// otherwise" visits the tree in depth-first order with no stack: the radix tree's depth is bounded only by the key length (64), and a
// runtime-indexed per-thread stack would live in scratch memory.
// Triangles are pre-gathered [F][3][3] in leaf order; a zero-area triangle is stored as NaNs, which fail every comparison below.
#pragma once
#include "d3h_vec.h"

namespace {

constexpr float BVH_INF = 3.0e38f;

struct BvhRay {
    V3 o, d, inv;
    float tmin, tmax;
};

__device__ __forceinline__ BvhRay bvh_make_ray(V3 o, V3 d, float tmin, float tmax) {
    BvhRay r;
    r.o = o; r.d = d;
    r.inv = mk(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);      // +-inf for a zero component: never multiplied (bvh_slab)
    r.tmin = tmin; r.tmax = tmax;
    return r;
}

// One axis of the slab test.  A direction component that is exactly zero (either sign) constrains nothing while the origin lies between the
// planes and rejects the box otherwise: (lo - o) * inf would be NaN for an origin ON a plane.
__device__ __forceinline__ void bvh_slab(float lo, float hi, float o, float d, float inv, float& tn, float& tf) {
    float t0 = (lo - o) * inv, t1 = (hi - o) * inv;
    bool zero = d == 0.0f;
    bool in = o >= lo && o <= hi;
    float a = zero ? (in ? -BVH_INF : BVH_INF) : fminf(t0, t1);
    float b = zero ? BVH_INF : fmaxf(t0, t1);
    tn = fmaxf(tn, a);
    tf = fminf(tf, b);
}

// the exit distance is widened by 2^-21 (the three roundings of each plane distance): a box may be entered needlessly, never missed
__device__ __forceinline__ bool bvh_hit_box(const BvhRay& r, float4 a, float4 b) {
    float tn = r.tmin, tf = r.tmax;
    bvh_slab(a.x, b.x, r.o.x, r.d.x, r.inv.x, tn, tf);
    bvh_slab(a.y, b.y, r.o.y, r.d.y, r.inv.y, tn, tf);
    bvh_slab(a.z, b.z, r.o.z, r.d.z, r.inv.z, tn, tf);
    return tn <= tf * 1.0000005f + 1e-30f;
}

// Moeller-Trumbore, two-sided, tmin <= t <= tmax
__device__ __forceinline__ bool bvh_hit_tri(const BvhRay& r, const float* __restrict__ t9) {
    V3 v0 = ld3(t9), e1 = ld3(t9 + 3) - v0, e2 = ld3(t9 + 6) - v0;
    V3 p = cross(r.d, e2);
    float det = dot(e1, p);
    float inv = 1.0f / det;
    V3 tv = r.o - v0;
    float u = dot(tv, p) * inv;
    V3 q = cross(tv, e1);
    float v = dot(r.d, q) * inv;
    float t = dot(e2, q) * inv;
    return fabsf(det) > 0.0f && u >= 0.0f && v >= 0.0f && u + v <= 1.0f && t >= r.tmin && t <= r.tmax;
}

// true if any triangle is crossed at tmin <= t <= tmax.  nodes: 2 float4 per node, tris: [F][9]; F = 0 is the empty scene.
__device__ __forceinline__ bool bvh_any_hit(const float4* __restrict__ nodes, const float* __restrict__ tris, int F, V3 o, V3 d, float tmin, float tmax) {
    if (F <= 0) return false;
    const BvhRay r = bvh_make_ray(o, d, tmin, tmax);
    int n = 0;
    while (n >= 0) {
        const float4 a = nodes[2 * (size_t)n], b = nodes[2 * (size_t)n + 1];
        const int link = __float_as_int(a.w), rope = __float_as_int(b.w);
        if (!bvh_hit_box(r, a, b)) { n = rope; continue; }
        if (link >= 0) { n = link; continue; }
        if (bvh_hit_tri(r, tris + 9 * (size_t)(~link))) return true;
        n = rope;
    }
    return false;
}

}  // namespace
