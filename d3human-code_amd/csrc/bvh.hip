// bvh.hip -- a triangle BVH built on the device, and the any-hit ("is this ray occluded by the mesh") query on it.
//
// Replaces (reference file:line): render/optixutils/c_src/optix_wrapper.cpp (optix_build_bvh: the OptiX acceleration structure) and the
// optixTrace of render/optixutils/c_src/envsampling/kernel.cu:101-118 (shadow_test: any-hit, terminate on first hit).  There is no ray-tracing
// hardware or library underneath: the build is a linear BVH (30-bit Morton codes of the centroids, sorted by the caller, a radix-tree hierarchy
// after Karras 2012 in one kernel, a bottom-up refit with one arrival counter per internal node), the traversal is stackless (d3h_bvh_dev.h).
//
// Build, in the caller's order:  d3h_bvh_build(phase 0) writes the 64-bit keys (code << 32 | triangle index: equal codes get distinct keys);
// the caller sorts them (torch.sort); d3h_bvh_build(phase 1) builds nodes and leaf-ordered triangles from the sorted keys.
#include "d3h_bvh_dev.h"

namespace {

__device__ __forceinline__ unsigned expand10(unsigned v) {      // 10 bits -> every third bit of 30
    v = (v * 0x00010001u) & 0xFF0000FFu;
    v = (v * 0x00000101u) & 0x0F00F00Fu;
    v = (v * 0x00000011u) & 0xC30C30C3u;
    v = (v * 0x00000005u) & 0x49249249u;
    return v;
}

__device__ __forceinline__ V3 tri_vertex(const float* __restrict__ verts, int V, long long idx) {
    idx = idx < 0 ? 0 : (idx >= V ? V - 1 : idx);            // an index outside the vertex array must not become a wild read
    return ld3(verts + 3 * idx);
}
__device__ __forceinline__ long long tri_index(const void* __restrict__ tris, int wide, size_t k) {
    return wide ? ((const long long*)tris)[k] : (long long)((const int*)tris)[k];
}

// cbounds: {min x, y, z, max x, y, z} of the centroids
__global__ __launch_bounds__(256) void bvh_keys_kernel(const float* __restrict__ verts, int V, const void* __restrict__ tris, int wide, int F,
                                                       const float* __restrict__ cbounds, long long* __restrict__ keys) {
    int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    V3 c = (tri_vertex(verts, V, tri_index(tris, wide, 3 * (size_t)f)) + tri_vertex(verts, V, tri_index(tris, wide, 3 * (size_t)f + 1)) +
            tri_vertex(verts, V, tri_index(tris, wide, 3 * (size_t)f + 2))) * (1.0f / 3.0f);
    float q[3] = {c.x, c.y, c.z};
    unsigned code = 0;
    for (int k = 0; k < 3; ++k) {
        float ext = cbounds[3 + k] - cbounds[k];
        float u = ext > 0.0f ? (q[k] - cbounds[k]) / ext : 0.0f;
        int cell = (int)fminf(fmaxf(u * 1024.0f, 0.0f), 1023.0f);      // a NaN centroid lands in cell 0
        code |= expand10((unsigned)cell) << (2 - k);
    }
    keys[f] = ((long long)code << 32) | (long long)f;
}

// length of the common prefix of keys i and j, -1 outside the array (the keys are distinct, so the XOR is never 0)
__device__ __forceinline__ int delta(const long long* __restrict__ keys, int F, int i, int j) {
    if (j < 0 || j >= F) return -1;
    return __clzll(keys[i] ^ keys[j]);
}

// Thread i < F - 1: internal node i of the radix tree (its children and their parent entries).  Thread j < F: leaf j (triangle gathered in
// Morton order, its box).  work: parent [2F-1], right child [F-1], arrival counter [F-1] (zero on entry).
__global__ __launch_bounds__(256) void bvh_hierarchy_kernel(const float* __restrict__ verts, int V, const void* __restrict__ tris, int wide, int F,
                                                            const long long* __restrict__ keys, float4* nodes, float* __restrict__ tri9,
                                                            int* parent, int* right) {
    int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= F) return;
    {   // leaf i
        long long f = keys[i] & 0xffffffffll;
        f = f >= F ? F - 1 : f;
        V3 a = tri_vertex(verts, V, tri_index(tris, wide, 3 * (size_t)f)), b = tri_vertex(verts, V, tri_index(tris, wide, 3 * (size_t)f + 1)),
           c = tri_vertex(verts, V, tri_index(tris, wide, 3 * (size_t)f + 2));
        V3 e1 = b - a, e2 = c - a, n = cross(e1, e2);
        // zero area: the sine of the angle at the first vertex is below 1e-6 (an edge of length 0 included); NaN vertices as well
        bool live = dot(n, n) > 1e-12f * dot(e1, e1) * dot(e2, e2);
        float* t = tri9 + 9 * (size_t)i;
        const float nan = __int_as_float(0x7fc00000);
        if (live) { st3(t, a); st3(t + 3, b); st3(t + 6, c); }
        else for (int k = 0; k < 9; ++k) t[k] = nan;
        float4 lo, hi;
        if (live) {
            lo = make_float4(fminf(a.x, fminf(b.x, c.x)), fminf(a.y, fminf(b.y, c.y)), fminf(a.z, fminf(b.z, c.z)), __int_as_float(~i));
            hi = make_float4(fmaxf(a.x, fmaxf(b.x, c.x)), fmaxf(a.y, fmaxf(b.y, c.y)), fmaxf(a.z, fmaxf(b.z, c.z)), __int_as_float(-1));
        } else {    // an empty box: the neutral element of the refit's min / max, rejected by every ray that has a non-zero direction component
            lo = make_float4(BVH_INF, BVH_INF, BVH_INF, __int_as_float(~i));
            hi = make_float4(-BVH_INF, -BVH_INF, -BVH_INF, __int_as_float(-1));
        }
        nodes[2 * (size_t)(F - 1 + i)] = lo;
        nodes[2 * (size_t)(F - 1 + i) + 1] = hi;
        if (F == 1) parent[0] = -1;
    }
    if (i >= F - 1) return;
    // internal node i covers the keys [min(i, j), max(i, j)]
    int d = delta(keys, F, i, i + 1) - delta(keys, F, i, i - 1) >= 0 ? 1 : -1;
    int dmin = delta(keys, F, i, i - d);
    int lmax = 2;
    while (delta(keys, F, i, i + lmax * d) > dmin) lmax *= 2;
    int l = 0;
    for (int t = lmax >> 1; t >= 1; t >>= 1)
        if (delta(keys, F, i, i + (l + t) * d) > dmin) l += t;
    int j = i + l * d;
    int dnode = delta(keys, F, i, j);
    int s = 0, t = l;
    do {
        t = (t + 1) >> 1;
        if (delta(keys, F, i, i + (s + t) * d) > dnode) s += t;
    } while (t > 1);
    int gamma = i + s * d + (d < 0 ? -1 : 0);
    int lo = i < j ? i : j, hi = i < j ? j : i;
    int left = lo == gamma ? F - 1 + gamma : gamma;
    int rgt = hi == gamma + 1 ? F - 1 + gamma + 1 : gamma + 1;
    nodes[2 * (size_t)i].w = __int_as_float(left);
    right[i] = rgt;
    parent[left] = i;
    parent[rgt] = i;
    if (i == 0) parent[0] = -1;
}

// Thread n < 2F - 1: the rope of node n (walk up to the first ancestor-or-self that is a left child: its right sibling).  A leaf thread then
// carries its box upwards; of the two threads that arrive at an internal node the second one, which finds both children complete, goes on.
// The first arriver's stores are published by the fence in front of its counter add, the second's loads are ordered behind its own.
__global__ __launch_bounds__(256) void bvh_refit_kernel(int F, float4* nodes, const int* __restrict__ parent, const int* __restrict__ right,
                                                        int* counter) {
    int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= 2 * F - 1) return;
    int rope = -1;
    for (int c = n, p = parent[n]; p >= 0; c = p, p = parent[p]) {
        if (right[p] != c) { rope = right[p]; break; }
    }
    nodes[2 * (size_t)n + 1].w = __int_as_float(rope);
    if (n < F - 1) return;
    int p = parent[n];
    while (p >= 0) {
        __threadfence();
        if (atomicAdd(counter + p, 1) == 0) return;
        __threadfence();
        int l = __float_as_int(nodes[2 * (size_t)p].w), r = right[p];
        float4 la = nodes[2 * (size_t)l], lb = nodes[2 * (size_t)l + 1], ra = nodes[2 * (size_t)r], rb = nodes[2 * (size_t)r + 1];
        float* a = (float*)(nodes + 2 * (size_t)p);
        float* b = (float*)(nodes + 2 * (size_t)p + 1);
        a[0] = fminf(la.x, ra.x); a[1] = fminf(la.y, ra.y); a[2] = fminf(la.z, ra.z);        // .w (link / rope) belongs to other stores
        b[0] = fmaxf(lb.x, rb.x); b[1] = fmaxf(lb.y, rb.y); b[2] = fmaxf(lb.z, rb.z);
        p = parent[p];
    }
}

__global__ __launch_bounds__(256) void bvh_occluded_kernel(const float4* __restrict__ nodes, const float* __restrict__ tri9, int F,
                                                           const float* __restrict__ org, const float* __restrict__ dir, size_t nrays,
                                                           float tmin, float tmax, unsigned char* __restrict__ out) {
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nrays) return;
    out[i] = bvh_any_hit(nodes, tri9, F, ld3(org + 3 * i), ld3(dir + 3 * i), tmin, tmax) ? 1 : 0;
}

}  // namespace

// Buffer sizes of a BVH over F triangles, HOST array sizes[4]: {floats of `nodes` (8 per node, 2F - 1 nodes, 16-byte aligned), floats of `tri9` (9 F),
// ints of `work` (4 F), int64 of `keys` (F)}.  F = 0: all zero.
extern "C" int d3h_bvh_layout(int64_t F, int64_t* sizes) {
    if (F < 0 || F > (1ll << 30) || !sizes) return D3H_ERR_ARG;
    sizes[0] = F > 0 ? 8 * (2 * F - 1) : 0;
    sizes[1] = 9 * F;
    sizes[2] = 4 * F;
    sizes[3] = F;
    return D3H_OK;
}
// Build the BVH of the mesh verts [V][3], tris [F][3] (int32, or int64 if tris_int64; an index outside [0, V) is clamped).  phase 0: keys [F] :=
// (30-bit Morton code of the centroid inside cbounds {min xyz, max xyz of the centroids}) << 32 | triangle index; the caller sorts keys
// ascending; phase 1: nodes, tri9 (triangles in leaf order, zero-area ones as NaN) and work are overwritten from the sorted keys.  F = 0 or V = 0:
// nothing is launched.  Only nodes, tri9 and F are needed afterwards.
extern "C" int d3h_bvh_build(int phase, const float* verts, int64_t V, const void* tris, int tris_int64, int64_t F, const float* cbounds, int64_t* keys,
                             float* nodes, float* tri9, int* work, void* stream) {
    if (phase < 0 || phase > 1 || V < 0 || F < 0 || F > (1ll << 30) || V > 0x7fffffffll) return D3H_ERR_ARG;
    if (F == 0 || V == 0) return D3H_OK;
    if (!verts || !tris || !keys) return D3H_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    const unsigned gf = (unsigned)((F + 255) / 256);
    if (phase == 0) {
        if (!cbounds) return D3H_ERR_ARG;
        hipLaunchKernelGGL(bvh_keys_kernel, dim3(gf), dim3(256), 0, s, verts, (int)V, tris, tris_int64, (int)F, cbounds, (long long*)keys);
        D3H_LAUNCH_CHECK();
        return D3H_OK;
    }
    if (!nodes || !tri9 || !work) return D3H_ERR_ARG;
    int* parent = work;
    int* right = work + (2 * F - 1);
    int* counter = work + (3 * F - 1);
    if (F > 1) {
        hipError_t e = hipMemsetAsync(counter, 0, sizeof(int) * (size_t)(F - 1), s);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(bvh_hierarchy_kernel, dim3(gf), dim3(256), 0, s, verts, (int)V, tris, tris_int64, (int)F, (const long long*)keys, (float4*)nodes,
                       tri9, parent, right);
    D3H_LAUNCH_CHECK();
    hipLaunchKernelGGL(bvh_refit_kernel, dim3((unsigned)((2 * F - 1 + 255) / 256)), dim3(256), 0, s, (int)F, (float4*)nodes, (const int*)parent,
                       (const int*)right, counter);
    D3H_LAUNCH_CHECK();
    return D3H_OK;
}
// out [nrays] (bytes, 0 / 1) := 1 where the ray org + t dir crosses a triangle of the BVH (nodes, tri9 of d3h_bvh_build, F) at tmin <= t <= tmax:
// any-hit, two-sided, zero-area triangles never hit.  F = 0 (nodes, tri9 may be NULL): all 0.
extern "C" int d3h_bvh_occluded(const float* nodes, const float* tri9, int64_t F, const float* org, const float* dir, int64_t nrays, float tmin, float tmax,
                                unsigned char* out, void* stream) {
    if (F < 0 || nrays < 0 || (F > 0 && (!nodes || !tri9))) return D3H_ERR_ARG;
    if (nrays == 0) return D3H_OK;
    if (!org || !dir || !out) return D3H_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(bvh_occluded_kernel, dim3((unsigned)((nrays + 255) / 256)), dim3(256), 0, s, (const float4*)nodes, tri9, (int)F, org, dir,
                       (size_t)nrays, tmin, tmax, out);
    D3H_LAUNCH_CHECK();
    return D3H_OK;
}
