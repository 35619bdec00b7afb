// bvhdist.hip -- distance queries on the triangle BVH of bvh.hip: the nearest triangle to a point, and the winding-signed distance with a
// hierarchical generalised winding number (Barill, Dickson, Schmidt, Levin, Jacobson 2018, "Fast winding numbers for soups and clouds", first order).
//
// Replaces what the reference asks pysdf for (geometry/hmsdf.py:236-237, script/process_body_cloth_head_msdfcut.py:683,744): pysdf answers from a
// spatial tree, the brute-force kernels of mesh_ops.hip loop over every triangle.  Here a query costs O(log F): the per-triangle arithmetic is that of
// the brute-force kernels (d3h_meshdist_dev.h), the traversal is the stackless rope walk of d3h_bvh_dev.h -- no runtime-indexed private array, no scratch.
//
// Node moments (d3h_bvh_moments), two float4 per node next to `nodes`:
//     {c.x, c.y, c.z, r}      c: area-weighted mean of the triangle centroids below the node (the box centre if the area is 0);
//                             r: distance from c to the farthest corner of the node's box, so every point of every triangle below lies within r of c
//     {n.x, n.y, n.z, area}   n: sum of the area vectors (e1 x e2) / 2; area: sum of their lengths.  Zero-area leaves (NaN rows of tri9) count as 0.
// A node none of whose triangles is live has the empty box of bvh.hip: c = 0, r = 0, n = 0.
#include "d3h_bvh_dev.h"
#include "d3h_meshdist_dev.h"

namespace {

__device__ __forceinline__ bool box_empty(float4 a, float4 b) { return a.x > b.x; }

// c and r of a node from its summed moments (sc = sum of area * centroid) and its box
__device__ __forceinline__ float4 moment_centre(V3 sc, float area, float4 a, float4 b) {
    if (box_empty(a, b)) return make_float4(0.f, 0.f, 0.f, 0.f);
    V3 c = area > 0.f ? sc * (1.0f / area) : mk(0.5f * (a.x + b.x), 0.5f * (a.y + b.y), 0.5f * (a.z + b.z));
    float fx = fmaxf(fabsf(c.x - a.x), fabsf(b.x - c.x)), fy = fmaxf(fabsf(c.y - a.y), fabsf(b.y - c.y)), fz = fmaxf(fabsf(c.z - a.z), fabsf(b.z - c.z));
    return make_float4(c.x, c.y, c.z, sqrtf(fx * fx + fy * fy + fz * fz));
}

// Thread j < F: the moments of leaf j, then upwards as bvh_refit_kernel goes: of the two threads that arrive at an internal node the second one, which
// finds both children complete, combines them and goes on.  The first arriver's stores are published by the fence in front of its counter add, the
// second's loads are ordered behind its own.  A node's value is a function of its two children's alone, whichever thread computes it.
// work: parent [2F-1], right child [F-1], arrival counter [F-1] (zero on entry), as bvh_hierarchy_kernel left the first two.
__global__ __launch_bounds__(256) void bvh_moments_kernel(int F, const float4* __restrict__ nodes, const float* __restrict__ tri9,
                                                          const int* __restrict__ parent, const int* __restrict__ right, int* counter, float4* mom) {
    int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= F) return;
    {
        const float* t = tri9 + 9 * (size_t)j;
        V3 a = ld3(t), b = ld3(t + 3), c = ld3(t + 6);
        V3 n = cross(b - a, c - a) * 0.5f;
        float area = sqrtf(dot(n, n));
        if (!(area > 0.f)) { n = mk(0.f, 0.f, 0.f); area = 0.f; }               // a NaN row as well
        V3 sc = area > 0.f ? (a + b + c) * (1.0f / 3.0f) * area : mk(0.f, 0.f, 0.f);
        size_t m = (size_t)(F - 1 + j);
        mom[2 * m] = moment_centre(sc, area, nodes[2 * m], nodes[2 * m + 1]);
        mom[2 * m + 1] = make_float4(n.x, n.y, n.z, area);
    }
    int p = parent[F - 1 + j];
    while (p >= 0) {
        __threadfence();
        if (atomicAdd(counter + p, 1) == 0) return;
        __threadfence();
        const float4 pa = nodes[2 * (size_t)p], pb = nodes[2 * (size_t)p + 1];
        int l = __float_as_int(pa.w), r = right[p];
        float4 lc = mom[2 * (size_t)l], ln = mom[2 * (size_t)l + 1], rc = mom[2 * (size_t)r], rn = mom[2 * (size_t)r + 1];
        float area = ln.w + rn.w;
        V3 sc = mk(lc.x, lc.y, lc.z) * ln.w + mk(rc.x, rc.y, rc.z) * rn.w;
        mom[2 * (size_t)p] = moment_centre(sc, area, pa, pb);
        mom[2 * (size_t)p + 1] = make_float4(ln.x + rn.x, ln.y + rn.y, ln.z + rn.z, area);
        p = parent[p];
    }
}

// squared distance of p to the box (0 inside), and to the box's farthest corner; an empty box (lo = BVH_INF) is infinitely far
__device__ __forceinline__ float box_dist2(V3 p, float4 a, float4 b, float& far2) {
    float nx = fmaxf(fmaxf(a.x - p.x, p.x - b.x), 0.f), ny = fmaxf(fmaxf(a.y - p.y, p.y - b.y), 0.f), nz = fmaxf(fmaxf(a.z - p.z, p.z - b.z), 0.f);
    float fx = fmaxf(p.x - a.x, b.x - p.x), fy = fmaxf(p.y - a.y, b.y - p.y), fz = fmaxf(p.z - a.z, b.z - p.z);
    far2 = fx * fx + fy * fy + fz * fz;
    return nx * nx + ny * ny + nz * nz;
}
// May the subtree of this box be skipped when `best` is the smallest squared distance so far?  The box distance is a lower bound of the exact distance to
// anything inside; what is compared with `best`, though, are ROUNDED triangle distances, and the rounded box distance.  The test is widened on both
// counts, the way bvh_hit_box widens its exit distance: by 2^-21 relative for the roundings of the box distance itself, and by 2^-20 of the squared
// distance to the box's farthest corner for tri_dist2, whose closest point carries an absolute error of a few ulps of the query-to-vertex distances
// (which the farthest corner bounds).  A box may be entered needlessly, never skipped wrongly; equality enters (a tie may hide a smaller index).
__device__ __forceinline__ bool box_skip(V3 p, float4 a, float4 b, float best) {
    if (box_empty(a, b)) return true;
    float far2;
    float d2 = box_dist2(p, a, b, far2);
    return d2 > best * 1.0000005f + 9.5367432e-7f * far2 + 1e-30f;
}

struct NearHit { float d2; int leaf, tri; };

__device__ __forceinline__ void near_leaf(NearHit& h, V3 p, const float* __restrict__ tri9, const int* __restrict__ leaf_tri, int j) {
    const float* t = tri9 + 9 * (size_t)j;
    V3 a = ld3(t);
    float d = tri_dist2(p, a, ld3(t + 3) - a, ld3(t + 6) - a);               // NaN for a zero-area triangle: both comparisons fail
    int o = leaf_tri ? leaf_tri[j] : j;
    if (d < h.d2 || (d == h.d2 && o < h.tri)) { h.d2 = d; h.leaf = j; h.tri = o; }
}

// The nearest triangle of p: its squared distance, its row of tri9 and its original index (d2 = inf, -1, -1 if there is none).  One greedy descent towards
// the nearer child's box gives the first bound, the rope walk then visits every node whose box is not farther than the best so far -- each node at
// most once, so the loop ends after at most 2F - 1 steps.  Ties in d2 go to the smallest original index: a first-minimum-wins loop over the triangles.
__device__ __forceinline__ NearHit bvh_nearest(const float4* __restrict__ nodes, const float* __restrict__ tri9, const int* __restrict__ leaf_tri, int F, V3 p) {
    NearHit h;
    h.d2 = INFINITY; h.leaf = -1; h.tri = -1;
    if (F <= 0 || !(fabsf(p.x) <= 3.0e38f && fabsf(p.y) <= 3.0e38f && fabsf(p.z) <= 3.0e38f)) return h;
    int n = 0;
    for (int link = __float_as_int(nodes[0].w); link >= 0; link = __float_as_int(nodes[2 * (size_t)n].w)) {
        int l = link, r = __float_as_int(nodes[2 * (size_t)l + 1].w);           // the right child is the rope of the left one
        float fl, fr;
        float dl = box_dist2(p, nodes[2 * (size_t)l], nodes[2 * (size_t)l + 1], fl), dr = box_dist2(p, nodes[2 * (size_t)r], nodes[2 * (size_t)r + 1], fr);
        n = dr < dl ? r : l;
    }
    near_leaf(h, p, tri9, leaf_tri, ~__float_as_int(nodes[2 * (size_t)n].w));
    n = 0;
    while (n >= 0) {
        const float4 a = nodes[2 * (size_t)n], b = nodes[2 * (size_t)n + 1];
        const int link = __float_as_int(a.w), rope = __float_as_int(b.w);
        if (box_skip(p, a, b, h.d2)) { n = rope; continue; }
        if (link >= 0) { n = link; continue; }
        near_leaf(h, p, tri9, leaf_tri, ~link);
        n = rope;
    }
    return h;
}

__global__ __launch_bounds__(256) void bvh_nearest_kernel(const float4* __restrict__ nodes, const float* __restrict__ tri9, const int* __restrict__ leaf_tri,
                                                          int F, const float* __restrict__ pts, size_t np, float* __restrict__ d2, int* __restrict__ tri,
                                                          float* __restrict__ bary) {
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= np) return;
    const V3 p = ld3(pts + 3 * i);
    const NearHit h = bvh_nearest(nodes, tri9, leaf_tri, F, p);
    V3 w = mk(0.f, 0.f, 0.f);
    if (h.leaf >= 0) {
        const float* t = tri9 + 9 * (size_t)h.leaf;
        V3 a = ld3(t);
        w = tri_closest_bary(p, a, ld3(t + 3) - a, ld3(t + 6) - a);
    }
    if (d2) d2[i] = h.d2;
    if (tri) tri[i] = h.tri;
    if (bary) st3(bary + 3 * i, w);
}

// Solid angle of the whole mesh seen from p, in radians, by the tree: a node whose centre is farther than beta * r contributes the dipole of its area
// vector, n . (c - p) / |c - p|^3, and its subtree is skipped; any other internal node is opened; a leaf contributes its exact angle as mesh_wsdf_kernel
// forms it (`fix`: what the float64 repair of the triangles in whose plane p lies changes).  beta = inf: (inf * r)^2 is never exceeded, every node is opened.
__device__ __forceinline__ void bvh_winding(const float4* __restrict__ nodes, const float* __restrict__ tri9, const float4* __restrict__ mom, int F, V3 p,
                                            float beta, float& wind, float& fix) {
    wind = 0.f; fix = 0.f;
    int n = F > 0 ? 0 : -1;
    while (n >= 0) {
        const int link = __float_as_int(nodes[2 * (size_t)n].w), rope = __float_as_int(nodes[2 * (size_t)n + 1].w);
        if (link >= 0) {
            const float4 m = mom[2 * (size_t)n];
            V3 d = mk(m.x, m.y, m.z) - p;
            float d2 = dot(d, d), br = beta * m.w;
            if (d2 > br * br) {                                                  // false for a NaN on either side: opened
                const float4 nn = mom[2 * (size_t)n + 1];
                wind += dot(mk(nn.x, nn.y, nn.z), d) / (d2 * sqrtf(d2));
                n = rope;
            } else n = link;
            continue;
        }
        const float* t = tri9 + 9 * (size_t)(~link);
        V3 a = ld3(t);
        if (a.x == a.x) {                                                        // a zero-area triangle is a row of NaNs
            const VosTerm s = vos_term(p, a, ld3(t + 3) - a, ld3(t + 6) - a);
            const float ang = 2.0f * atan2f(s.det, s.den);
            wind += ang;
            if (fabsf(s.det) < 1e-4f * s.lll) fix += wsdf_angle_f64(p, t, t + 3, t + 6) - ang;
        }
        n = rope;
    }
}

__global__ __launch_bounds__(256) void bvh_wsdf_kernel(const float4* __restrict__ nodes, const float* __restrict__ tri9, const float4* __restrict__ mom, int F,
                                                       const float* __restrict__ pts, size_t np, float beta, float* __restrict__ out_sdf,
                                                       float* __restrict__ out_w) {
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= np) return;
    const V3 p = ld3(pts + 3 * i);
    float wind, fix;
    bvh_winding(nodes, tri9, mom, F, p, beta, wind, fix);
    // the inside rule and the 1e-3 rad rule of mesh_wsdf_kernel
    const float rep = wind + fix;
    const bool inside = fabsf(fabsf(rep) - 6.2831853f) < 1e-3f ? fabsf(wind) > 6.2831853f : fabsf(rep) > 6.2831853f;
    if (out_w) out_w[i] = rep * 0.079577472f;                                           // 1 / (4 pi)
    if (out_sdf) {
        const float best = bvh_nearest(nodes, tri9, nullptr, F, p).d2;          // the nearest walk; without leaf_tri ties go by leaf order, which the distance does not see
        out_sdf[i] = (inside ? -1.0f : 1.0f) * sqrtf(best);
    }
}

}  // namespace

// moments [2F - 1][2][4] (16-byte aligned) := the node moments of the BVH (nodes, tri9, work of d3h_bvh_build, phase 1; F): per node {c.xyz, r},
// {n.xyz, area} -- n the sum of the triangles' area vectors, c the area-weighted mean of their centroids (the box centre if the area is 0), r the distance
// from c to the farthest corner of the node's box; zero-area triangles count as 0.  The arrival counters of `work` are reset and used.  F = 0: nothing.
extern "C" int d3h_bvh_moments(const float* nodes, const float* tri9, int* work, int64_t F, float* moments, void* stream) {
    if (F < 0 || F > (1ll << 30)) return D3H_ERR_ARG;
    if (F == 0) return D3H_OK;
    if (!nodes || !tri9 || !work || !moments) return D3H_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    const int* parent = work;
    const int* right = work + (2 * F - 1);
    int* counter = work + (3 * F - 1);
    if (F > 1) {
        hipError_t e = hipMemsetAsync(counter, 0, sizeof(int) * (size_t)(F - 1), s);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(bvh_moments_kernel, dim3((unsigned)((F + 255) / 256)), dim3(256), 0, s, (int)F, (const float4*)nodes, tri9, parent, right, counter,
                       (float4*)moments);
    D3H_LAUNCH_CHECK();
    return D3H_OK;
}
// Nearest triangle of each point pts [n][3] on the BVH (nodes, tri9 of d3h_bvh_build; leaf_tri [F]: the original index of the triangle in leaf j, the low
// 32 bits of the sorted keys).  d2 [n] := squared distance, tri [n] := ORIGINAL triangle index, bary [n][3] := weights of the closest point on that triangle's
// three vertices; each output may be NULL.  Exact: the minimum over all triangles of non-zero area of the brute-force kernels' tri_dist2, ties in d2 to the
// smallest index.  F = 0, no triangle of non-zero area, or a point with a non-finite coordinate: d2 = +inf, tri = -1, bary = 0.
extern "C" int d3h_bvh_nearest(const float* nodes, const float* tri9, const int* leaf_tri, int64_t F, const float* pts, int64_t n, float* d2, int* tri,
                               float* bary, void* stream) {
    if (F < 0 || F > (1ll << 30) || n < 0 || (F > 0 && (!nodes || !tri9 || !leaf_tri))) return D3H_ERR_ARG;
    if (n == 0) return D3H_OK;
    if (!pts) return D3H_ERR_ARG;
    hipLaunchKernelGGL(bvh_nearest_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const float4*)nodes, tri9, leaf_tri, (int)F,
                       pts, (size_t)n, d2, tri, bary);
    D3H_LAUNCH_CHECK();
    return D3H_OK;
}
// Winding-signed distance of each point pts [n][3] to the mesh of the BVH (nodes, tri9 of d3h_bvh_build; moments of d3h_bvh_moments), d3h_mesh_wsdf's
// outputs by the tree: w [n] := the generalised winding number in turns, a node whose centre c is farther than beta * r from the point taken as the
// dipole n . (c - q) / |c - q|^3 of its area vector, every other node opened, a leaf exact (beta = +inf: the exact sum, in tree order); sdf [n] :=
// (|w| > 0.5 ? -1 : +1) * distance to the nearest triangle, d3h_mesh_wsdf's inside rule.  Either output may be NULL.  beta > 0.  F = 0: w = 0, sdf = +inf.
extern "C" int d3h_bvh_wsdf(const float* nodes, const float* tri9, const float* moments, int64_t F, const float* pts, int64_t n, float beta, float* sdf,
                            float* w, void* stream) {
    if (F < 0 || F > (1ll << 30) || n < 0 || !(beta > 0.0f) || (F > 0 && (!nodes || !tri9 || !moments))) return D3H_ERR_ARG;
    if (n == 0 || (!sdf && !w)) return D3H_OK;
    if (!pts) return D3H_ERR_ARG;
    hipLaunchKernelGGL(bvh_wsdf_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const float4*)nodes, tri9,
                       (const float4*)moments, (int)F, pts, (size_t)n, beta, sdf, w);
    D3H_LAUNCH_CHECK();
    return D3H_OK;
}
