// raster.hip -- differentiable rasterize / interpolate / antialias / texture for gfx950.
//
// Replaces the nvdiffrast calls of the reference (un-vendored third party, README.md:29; call sites
// render/render.py:37 interpolate, :72,:102 texture, :381 antialias, :400-403 DepthPeeler.rasterize_next_layer).
// nvdiffrast's source is not in the reference tree, so the semantics below are this build's restatement of its
// published behaviour ("parity unpinned" for these four ops -- they are pinned against
// oracle/raster.py instead):
//   rasterize  : clip-space triangles -> per pixel (u, v, z/w, triangle_id + 1) and (du/dX, du/dY, dv/dX, dv/dY) in pixel
//                units; pixel (x, y) samples NDC ((x+.5)/W*2-1, (y+.5)/H*2-1); nearest z/w wins, ties -> lower id;
//                u, v are the perspective-correct barycentrics of vertices 0 and 1; triangles that cross the camera plane are
//                rasterised with the homogeneous form of the edge functions (no explicit clipping), the depth range removes what
//                lies in front of the near plane.
//   interpolate: out = u a0 + v a1 + (1-u-v) a2, zero where empty; optional attribute pixel derivatives.
//   antialias  : for 4-neighbour pixel pairs with different ids, blend across the silhouette edge of the nearer
//                triangle by where it crosses the segment between the two pixel centres (an edge is only considered by
//                the pair axis it is closer to perpendicular to, which bounds d(crossing)/d(vertex) by 1); gradients to
//                colour and positions.
//   texture    : bilinear, clamp, texel centres at (i+.5)/N.
//
// MI355X design notes: triangles are rasterised one WAVE each (wave-uniform set-up, 64 lanes sweep the bounding box) straight
// into a 64-bit (depth | id) buffer with atomicMin, then one coalesced per-pixel resolve pass computes barycentrics and
// derivatives.  All image-space passes are HBM-streaming: 16-B pixel records, NHWC, one pass each.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include "d3h_common.h"
#include "composite.h"

namespace {

struct TriSetup {
    float X[3], Y[3], q[3], zw[3];   // NDC x, y; 1/w; z/w
    bool ok;                         // every vertex in front of the camera plane (w > 1e-8): the common case
    bool cross;                      // some but not all: the triangle crosses the camera plane (see raster_pixel_cross)
};

__device__ __forceinline__ TriSetup load_tri(const float* __restrict__ pos, const int* __restrict__ tri, int f) {
    TriSetup t;
    int nfront = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        int vi = tri[3 * (size_t)f + k];
        float4 p = *(const float4*)(pos + 4 * (size_t)vi);
        if (p.w > 1e-8f) ++nfront;
        float w = (fabsf(p.w) < 1e-8f) ? ((p.w < 0.f) ? -1e-8f : 1e-8f) : p.w;      // a vertex exactly on the camera plane has no projection
        float q = 1.0f / w;
        t.q[k] = q;
        t.X[k] = p.x * q;
        t.Y[k] = p.y * q;
        t.zw[k] = p.z * q;
    }
    t.ok = nfront == 3;
    t.cross = nfront == 1 || nfront == 2;
    return t;
}

// edge functions of point (fx, fy): a_i = orient(p, v_{i+1}, v_{i+2})
__device__ __forceinline__ void edge_fn(const TriSetup& t, float fx, float fy, float (&a)[3]) {
    float x0 = t.X[0] - fx, y0 = t.Y[0] - fy, x1 = t.X[1] - fx, y1 = t.Y[1] - fy, x2 = t.X[2] - fx, y2 = t.Y[2] - fy;
    a[0] = x1 * y2 - y1 * x2;
    a[1] = x2 * y0 - y2 * x0;
    a[2] = x0 * y1 - y0 * x1;
}

__device__ __forceinline__ unsigned order_key(float z) {
    unsigned u = __float_as_uint(z);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// (depth | id) key of triangle f at pixel (px, py), or false when the pixel centre is not covered / outside the depth range
__device__ __forceinline__ bool raster_key(const TriSetup& t, float area, int px, int py, int W, int H, int f, unsigned long long& key) {
    float fx = (px + 0.5f) * (2.0f / W) - 1.0f, fy = (py + 0.5f) * (2.0f / H) - 1.0f;
    float a[3];
    edge_fn(t, fx, fy, a);
    bool in = (area > 0.f) ? (a[0] >= 0.f && a[1] >= 0.f && a[2] >= 0.f) : (a[0] <= 0.f && a[1] <= 0.f && a[2] <= 0.f);
    if (!in) return false;
    float s = a[0] + a[1] + a[2];
    if (s == 0.f) return false;
    float is = 1.0f / s;
    float zw = (a[0] * t.zw[0] + a[1] * t.zw[1] + a[2] * t.zw[2]) * is;
    if (!(zw >= -1.0f && zw <= 1.0f)) return false;
    key = ((unsigned long long)order_key(zw) << 32) | (unsigned)(f + 1);
    return true;
}
__device__ __forceinline__ void raster_pixel(const TriSetup& t, float area, int px, int py, int W, int H, int f,
                                             unsigned long long* __restrict__ zb) {
    unsigned long long key;
    if (raster_key(t, area, px, py, W, H, f, key)) atomicMin(&zb[(size_t)py * W + px], key);
}

// Near-plane crossing (some w <= 0): no explicit clipping, the homogeneous form of the same edge functions.  With n_k = a_k q_k the
// perspective-correct barycentrics are n_k / S whatever the signs of the q_k (their common factor q0 q1 q2 cancels -- which is also why
// the resolve and backward kernels need no change), the interpolated w is s / S and z/w is sum(a_k zw_k) / s.  Covered iff every
// barycentric is >= 0 and the interpolated w is > 0; the depth-range test then removes what lies in front of the near plane.
__device__ __forceinline__ bool raster_key_cross(const TriSetup& t, int px, int py, int W, int H, int f, unsigned long long& key) {
    float fx = (px + 0.5f) * (2.0f / W) - 1.0f, fy = (py + 0.5f) * (2.0f / H) - 1.0f;
    float a[3];
    edge_fn(t, fx, fy, a);
    float s = a[0] + a[1] + a[2];
    float n0 = a[0] * t.q[0], n1 = a[1] * t.q[1], n2 = a[2] * t.q[2];
    float S = (n0 + n1) + n2;
    bool in = (n0 * S >= 0.f) && (n1 * S >= 0.f) && (n2 * S >= 0.f) && S != 0.f && (s * S > 0.f) && (fabsf(S) <= 3.0e38f);      // (finite)
    if (!in || s == 0.f) return false;
    float is = 1.0f / s;
    float zw = (a[0] * t.zw[0] + a[1] * t.zw[1] + a[2] * t.zw[2]) * is;
    if (!(zw >= -1.0f && zw <= 1.0f)) return false;
    key = ((unsigned long long)order_key(zw) << 32) | (unsigned)(f + 1);
    return true;
}
__device__ __forceinline__ void raster_pixel_cross(const TriSetup& t, int px, int py, int W, int H, int f, unsigned long long* __restrict__ zb) {
    unsigned long long key;
    if (raster_key_cross(t, px, py, W, H, f, key)) atomicMin(&zb[(size_t)py * W + px], key);
}

// pixel bounding box of a front-facing-or-not triangle with every vertex in front of the camera plane; false when it covers no pixel centre
__device__ __forceinline__ bool tri_bbox(const TriSetup& t, int W, int H, float& area, int& x0, int& x1, int& y0, int& y1) {
    area = (t.X[1] - t.X[0]) * (t.Y[2] - t.Y[0]) - (t.Y[1] - t.Y[0]) * (t.X[2] - t.X[0]);
    if (area == 0.f) return false;
    float xmin = fminf(t.X[0], fminf(t.X[1], t.X[2])), xmax = fmaxf(t.X[0], fmaxf(t.X[1], t.X[2]));
    float ymin = fminf(t.Y[0], fminf(t.Y[1], t.Y[2])), ymax = fmaxf(t.Y[0], fmaxf(t.Y[1], t.Y[2]));
    // pixel px covers NDC centre (px+.5)*2/W-1  ->  px in [ceil((xmin+1)*W/2 - .5), floor((xmax+1)*W/2 - .5)]
    x0 = (int)fmaxf(0.f, ceilf((xmin + 1.0f) * 0.5f * W - 0.5f)); x1 = (int)fminf((float)(W - 1), floorf((xmax + 1.0f) * 0.5f * W - 0.5f));
    y0 = (int)fmaxf(0.f, ceilf((ymin + 1.0f) * 0.5f * H - 0.5f)); y1 = (int)fminf((float)(H - 1), floorf((ymax + 1.0f) * 0.5f * H - 0.5f));
    return x1 >= x0 && y1 >= y0;
}

// One WAVE per triangle, 16 consecutive triangles per wave: the triangle set-up is wave-uniform (scalar loads), the 64 lanes sweep
// the bounding box as 8x8 pixel blocks.  A marching-tets mesh at tet-res 128 has ~10^4 faces of ~10^2-10^3 pixels each at 1024^2,
// so a thread-per-triangle bounding-box loop is both divergent and serial; here every lane tests one pixel per step.
constexpr int TRIS_PER_WAVE = 16;

__global__ __launch_bounds__(256) void raster_tris_kernel(const float* __restrict__ pos, int nv, int pos_bstride,
                                                          const int* __restrict__ tri, int nf, int H, int W,
                                                          unsigned long long* __restrict__ zbuf, const int* __restrict__ binned_flag) {
    if (binned_flag && binned_flag[0]) return;          // the tile-binned path took this render (raster_tile_kernel)
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int b = blockIdx.y;
    const int base = (blockIdx.x * 4 + wave) * TRIS_PER_WAVE;
    const float* posb = pos + (size_t)b * pos_bstride;
    unsigned long long* zb = zbuf + (size_t)b * H * W;
    const int lx = lane & 7, ly = lane >> 3;
    const int fend = min(base + TRIS_PER_WAVE, nf);
    for (int f = base; f < fend; ++f) {
        TriSetup t = load_tri(posb, tri, f);
        if (t.cross) {                          // rare: the whole frame is its bounding box
            for (int by = 0; by < H; by += 8)
                for (int bx = 0; bx < W; bx += 8) {
                    int px = bx + lx, py = by + ly;
                    if (px < W && py < H) raster_pixel_cross(t, px, py, W, H, f, zb);
                }
            continue;
        }
        if (!t.ok) continue;                    // entirely behind the camera plane
        float area;
        int x0, x1, y0, y1;
        if (!tri_bbox(t, W, H, area, x0, x1, y0, y1)) continue;
        for (int by = y0; by <= y1; by += 8)
            for (int bx = x0; bx <= x1; bx += 8) {
                int px = bx + lx, py = by + ly;
                if (px <= x1 && py <= y1) raster_pixel(t, area, px, py, W, H, f, zb);
            }
    }
}

// per pixel: winning triangle -> (u, v, z/w, id+1) and (du/dX, du/dY, dv/dX, dv/dY)
__device__ __forceinline__ void resolve_pixel(const float* __restrict__ posb, const int* __restrict__ tri, unsigned long long key, int px, int py,
                                              int W, int H, float4& r, float4& d) {
    r = make_float4(0.f, 0.f, 0.f, 0.f);
    d = make_float4(0.f, 0.f, 0.f, 0.f);
    unsigned id = (unsigned)(key & 0xFFFFFFFFull);
    if (key != ~0ull && id != 0) {
        int f = (int)id - 1;
        TriSetup t = load_tri(posb, tri, f);
        float fx = (px + 0.5f) * (2.0f / W) - 1.0f, fy = (py + 0.5f) * (2.0f / H) - 1.0f;
        float a[3];
        edge_fn(t, fx, fy, a);
        float s = a[0] + a[1] + a[2];
        float zw = (a[0] * t.zw[0] + a[1] * t.zw[1] + a[2] * t.zw[2]) / s;
        float n0 = a[0] * t.q[0], n1 = a[1] * t.q[1], n2 = a[2] * t.q[2];
        float S = n0 + n1 + n2;
        float iS = 1.0f / S;
        float u = n0 * iS, v = n1 * iS;
        // d a_i / d fx = -(Y_{i+2} - Y_{i+1}) ... from a_i = (X_{i+1}-fx)(Y_{i+2}-fy) - (Y_{i+1}-fy)(X_{i+2}-fx)
        float dax[3] = {t.Y[1] - t.Y[2], t.Y[2] - t.Y[0], t.Y[0] - t.Y[1]};
        float day[3] = {t.X[2] - t.X[1], t.X[0] - t.X[2], t.X[1] - t.X[0]};
        float dnx[3] = {dax[0] * t.q[0], dax[1] * t.q[1], dax[2] * t.q[2]};
        float dny[3] = {day[0] * t.q[0], day[1] * t.q[1], day[2] * t.q[2]};
        float dSx = dnx[0] + dnx[1] + dnx[2], dSy = dny[0] + dny[1] + dny[2];
        float sx = 2.0f / W, sy = 2.0f / H;   // d fx / d pixel
        r = make_float4(u, v, zw, (float)id);
        d = make_float4((dnx[0] - u * dSx) * iS * sx, (dny[0] - u * dSy) * iS * sy, (dnx[1] - v * dSx) * iS * sx, (dny[1] - v * dSy) * iS * sy);
    }
}
__global__ __launch_bounds__(256) void raster_resolve_kernel(const float* __restrict__ pos, int pos_bstride, const int* __restrict__ tri,
                                                             int H, int W, int nb, const unsigned long long* __restrict__ zbuf,
                                                             float* __restrict__ rast, float* __restrict__ db, const int* __restrict__ binned_flag) {
    if (binned_flag && binned_flag[0]) return;
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    size_t n = (size_t)nb * H * W;
    if (i >= n) return;
    int b = (int)(i / ((size_t)H * W));
    int rem = (int)(i % ((size_t)H * W));
    float4 r, d;
    resolve_pixel(pos + (size_t)b * pos_bstride, tri, zbuf[i], rem % W, rem / W, W, H, r, d);
    *(float4*)(rast + 4 * i) = r;
    if (db) *(float4*)(db + 4 * i) = d;
}

// ------------------------------------------------------------------------------------------------
// depth peeling and range mode (the contract: d3h/raster.py's docstring)
// ------------------------------------------------------------------------------------------------
// Previous-layer keys, one thread per pixel: the (depth | id) key the previous layer's winner (rast.w) had at this pixel, RECOMPUTED with the
// device functions that chose it -- load_tri, then raster_key_cross, or tri_bbox's area and raster_key -- so it is the same arithmetic and the
// same bits as the key that won.  An empty pixel gets ~0 (nothing is admitted there any more), and so does an id outside [1, nf] or a key that
// does not recompute (neither can come from a layer of these pos / tri).  16 B read + 8 B written per pixel; no z-buffer is kept between layers.
__global__ __launch_bounds__(256) void raster_peel_key_kernel(const float* __restrict__ pos, int pos_bstride, const int* __restrict__ tri, int nf,
                                                              int H, int W, int nb, const float* __restrict__ prev_rast,
                                                              unsigned long long* __restrict__ prev_key) {
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    size_t n = (size_t)nb * H * W;
    if (i >= n) return;
    const float4 r = *(const float4*)(prev_rast + 4 * i);
    const int id = (int)r.w;
    unsigned long long key = ~0ull;
    if (id > 0 && id <= nf) {
        const int b = (int)(i / ((size_t)H * W));
        const int rem = (int)(i % ((size_t)H * W));
        const int px = rem % W, py = rem / W, f = id - 1;
        TriSetup t = load_tri(pos + (size_t)b * pos_bstride, tri, f);
        unsigned long long k;
        float area;
        int x0, x1, y0, y1;
        const bool ok = t.cross ? raster_key_cross(t, px, py, W, H, f, k)
                                : (t.ok && tri_bbox(t, W, H, area, x0, x1, y0, y1) && raster_key(t, area, px, py, W, H, f, k));
        if (ok) key = k;
    }
    prev_key[i] = key;
}

// raster_tris_kernel for a peeled layer and / or range mode (the wave path only; the tile-binned kernel is never used here).
//  - prev_key [nb][H][W] (or NULL): a fragment enters the atomicMin only if its key is STRICTLY greater than the previous layer's key at that
//    pixel; a lane reads its previous key only where the pixel is covered, so the 8 x 8 block reads them one 64-B row at a time.
//  - ranges [nb][2] = (start, count) (or NULL): frame b rasterises triangles start .. start + count - 1 of tri (the grid's x dimension is
//    sized by the largest count; the ids stay absolute); pos is then shared by every frame (pos_bstride = 0).  A range outside [0, nf]
//    rasterises nothing (the host refuses it before the launch).
__global__ __launch_bounds__(256) void raster_tris_peel_kernel(const float* __restrict__ pos, int pos_bstride, const int* __restrict__ tri, int nf,
                                                               const int* __restrict__ ranges, int H, int W,
                                                               const unsigned long long* __restrict__ prev_key, unsigned long long* __restrict__ zbuf) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int b = blockIdx.y;
    int start = 0, count = nf;
    if (ranges) {
        start = ranges[2 * b];
        count = ranges[2 * b + 1];
        if (start < 0 || count < 0 || start > nf - count) return;
    }
    const int local = (blockIdx.x * 4 + wave) * TRIS_PER_WAVE;
    const float* posb = pos + (size_t)b * pos_bstride;
    unsigned long long* zb = zbuf + (size_t)b * H * W;
    const unsigned long long* pk = prev_key ? prev_key + (size_t)b * H * W : nullptr;
    const int lx = lane & 7, ly = lane >> 3;
    const int fend = start + min(local + TRIS_PER_WAVE, count);
    for (int f = start + local; f < fend; ++f) {
        TriSetup t = load_tri(posb, tri, f);
        if (t.cross) {                          // rare: the whole frame is its bounding box
            for (int by = 0; by < H; by += 8)
                for (int bx = 0; bx < W; bx += 8) {
                    int px = bx + lx, py = by + ly;
                    unsigned long long key;
                    if (px < W && py < H && raster_key_cross(t, px, py, W, H, f, key)) {
                        const size_t o = (size_t)py * W + px;
                        if (!pk || key > pk[o]) atomicMin(&zb[o], key);
                    }
                }
            continue;
        }
        if (!t.ok) continue;                    // entirely behind the camera plane
        float area;
        int x0, x1, y0, y1;
        if (!tri_bbox(t, W, H, area, x0, x1, y0, y1)) continue;
        for (int by = y0; by <= y1; by += 8)
            for (int bx = x0; bx <= x1; bx += 8) {
                int px = bx + lx, py = by + ly;
                unsigned long long key;
                if (px <= x1 && py <= y1 && raster_key(t, area, px, py, W, H, f, key)) {
                    const size_t o = (size_t)py * W + px;
                    if (!pk || key > pk[o]) atomicMin(&zb[o], key);
                }
            }
    }
}

// ------------------------------------------------------------------------------------------------
// tile-binned rasteriser (large meshes)
// ------------------------------------------------------------------------------------------------
// The wave-per-triangle kernel above is right for the fitted meshes of this workload (~10^4 triangles of 10^2..10^3 pixels: 69 us for four
// 1024^2 frames); at 10^5..10^6 triangles of a few pixels each it spends 64 lanes and a 64-bit global atomic on every triangle (534 us at
// 593 k).  This path bins the triangles into 32 x 32-pixel tiles (count -> scan -> fill, bounding-box conservative), then ONE workgroup per
// tile keeps the tile's (depth | id) keys in LDS: small triangles are rasterised one per LANE, large ones one per WAVE, both with LDS
// atomic-min; the resolve of the tile's 1 024 pixels follows in the same kernel (no z-buffer in memory, no separate resolve pass).
// Same key arithmetic, same candidate set per pixel (the bounding boxes are the wave kernel's) -> bit-identical `rast` / `rast_db`.
// scratch (ints): cnt[NT] | off[NT + 1] | cur[NT] | flag[4] (0: binned path active, 1: pairs, 2: capacity) | pairs[cap];  NT = nb * tiles
constexpr int BIN_T = 32;

__device__ __forceinline__ bool bin_range(const TriSetup& t, int W, int H, int tx_n, int ty_n, int& tx0, int& tx1, int& ty0, int& ty1) {
    if (t.cross) { tx0 = 0; ty0 = 0; tx1 = tx_n - 1; ty1 = ty_n - 1; return true; }
    if (!t.ok) return false;
    float area;
    int x0, x1, y0, y1;
    if (!tri_bbox(t, W, H, area, x0, x1, y0, y1)) return false;
    tx0 = x0 / BIN_T; tx1 = x1 / BIN_T; ty0 = y0 / BIN_T; ty1 = y1 / BIN_T;
    return true;
}

// FILL = false: count the (triangle, tile) pairs per tile; FILL = true: write the triangle ids into the tiles' lists
template <bool FILL>
__global__ __launch_bounds__(256) void raster_bin_kernel(const float* __restrict__ pos, int pos_bstride, const int* __restrict__ tri, int nf, int H, int W,
                                                         int tx_n, int ty_n, int* __restrict__ cnt, const int* __restrict__ off, int* __restrict__ cur,
                                                         const int* __restrict__ flag, int* __restrict__ pairs) {
    if (FILL && !flag[0]) return;
    const int f = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (f >= nf) return;
    TriSetup t = load_tri(pos + (size_t)b * pos_bstride, tri, f);
    int tx0, tx1, ty0, ty1;
    if (!bin_range(t, W, H, tx_n, ty_n, tx0, tx1, ty0, ty1)) return;
    const int T = tx_n * ty_n;
    for (int ty = ty0; ty <= ty1; ++ty)
        for (int tx = tx0; tx <= tx1; ++tx) {
            const int tile = b * T + ty * tx_n + tx;
            if (FILL) pairs[off[tile] + atomicAdd(&cur[tile], 1)] = f;
            else atomicAdd(&cnt[tile], 1);
        }
}

// exclusive scan of cnt[NT] -> off[NT + 1] (one workgroup; NT is a few thousand), the decision and the cursors
__global__ __launch_bounds__(1024) void raster_bin_scan_kernel(const int* __restrict__ cnt, int NT, int* __restrict__ off, int* __restrict__ cur,
                                                               int* __restrict__ flag, int cap) {
    __shared__ int part[1024];
    const int tid = threadIdx.x;
    const int per = (NT + 1023) / 1024;
    int sum = 0;
    for (int k = 0; k < per; ++k) { int i = tid * per + k; if (i < NT) sum += cnt[i]; }
    part[tid] = sum;
    __syncthreads();
    for (int st = 1; st < 1024; st <<= 1) {
        int v = (tid >= st) ? part[tid - st] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    int run = part[tid] - sum;
    for (int k = 0; k < per; ++k) {
        int i = tid * per + k;
        if (i < NT) { off[i] = run; run += cnt[i]; cur[i] = 0; }
    }
    if (tid == 1023) {
        off[NT] = part[1023];
        flag[1] = part[1023];
        flag[2] = cap;
        flag[0] = part[1023] <= cap ? 1 : 0;          // does not fit: the wave-per-triangle path runs instead (it checks the same flag)
    }
}

__global__ __launch_bounds__(256) void raster_tile_kernel(const float* __restrict__ pos, int pos_bstride, const int* __restrict__ tri, int H, int W,
                                                          int tx_n, int ty_n, const int* __restrict__ off, const int* __restrict__ flag,
                                                          int* __restrict__ pairs, float* __restrict__ rast, float* __restrict__ db) {
    if (!flag[0]) return;
    __shared__ unsigned long long zt[BIN_T * BIN_T];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.y, tile = blockIdx.x;
    const int px0 = (tile % tx_n) * BIN_T, py0 = (tile / tx_n) * BIN_T;
    const int pxe = min(px0 + BIN_T, W) - 1, pye = min(py0 + BIN_T, H) - 1;          // last pixel of the tile inside the image
    const float* posb = pos + (size_t)b * pos_bstride;
    for (int i = tid; i < BIN_T * BIN_T; i += 256) zt[i] = ~0ull;
    __syncthreads();
    const int T = tx_n * ty_n;
    const int base = off[b * T + tile], n = off[b * T + tile + 1] - base;
    // phase A: one triangle per lane; a triangle whose box inside the tile is larger than 16 pixels (or that crosses the camera plane) is
    // left for phase B, marked by complementing its id in the tile's own list
    for (int i = tid; i < n; i += 256) {
        const int f = pairs[base + i];
        TriSetup t = load_tri(posb, tri, f);
        bool big = t.cross;
        if (!big) {
            float area;
            int x0, x1, y0, y1;
            if (!t.ok || !tri_bbox(t, W, H, area, x0, x1, y0, y1)) continue;          // (cannot happen: the binning used the same test)
            x0 = max(x0, px0); x1 = min(x1, pxe); y0 = max(y0, py0); y1 = min(y1, pye);
            if ((x1 - x0 + 1) * (y1 - y0 + 1) > 16) big = true;
            else
                for (int py = y0; py <= y1; ++py)
                    for (int px = x0; px <= x1; ++px) {
                        unsigned long long key;
                        if (raster_key(t, area, px, py, W, H, f, key)) atomicMin(&zt[(py - py0) * BIN_T + (px - px0)], key);
                    }
        }
        if (big) pairs[base + i] = ~f;
    }
    __syncthreads();
    // phase B: one large triangle per wave, 8 x 8 pixel blocks over its box inside the tile
    const int lx = lane & 7, ly = lane >> 3;
    for (int i = wave; i < n; i += 4) {
        const int v = pairs[base + i];          // (wave-uniform)
        if (v >= 0) continue;
        const int f = ~v;
        TriSetup t = load_tri(posb, tri, f);
        if (t.cross) {
            for (int by = py0; by <= pye; by += 8)
                for (int bx = px0; bx <= pxe; bx += 8) {
                    int px = bx + lx, py = by + ly;
                    unsigned long long key;
                    if (px <= pxe && py <= pye && raster_key_cross(t, px, py, W, H, f, key)) atomicMin(&zt[(py - py0) * BIN_T + (px - px0)], key);
                }
            continue;
        }
        float area;
        int x0, x1, y0, y1;
        if (!tri_bbox(t, W, H, area, x0, x1, y0, y1)) continue;
        x0 = max(x0, px0); x1 = min(x1, pxe); y0 = max(y0, py0); y1 = min(y1, pye);
        for (int by = y0; by <= y1; by += 8)
            for (int bx = x0; bx <= x1; bx += 8) {
                int px = bx + lx, py = by + ly;
                unsigned long long key;
                if (px <= x1 && py <= y1 && raster_key(t, area, px, py, W, H, f, key)) atomicMin(&zt[(py - py0) * BIN_T + (px - px0)], key);
            }
    }
    __syncthreads();
    // resolve: rows of 32 pixels x 16 B = 512 B, eight rows per pass
    for (int i = tid; i < BIN_T * BIN_T; i += 256) {
        const int px = px0 + (i % BIN_T), py = py0 + (i / BIN_T);
        if (px >= W || py >= H) continue;
        float4 r, d;
        resolve_pixel(posb, tri, zt[i], px, py, W, H, r, d);
        const size_t o = ((size_t)b * H + py) * W + px;
        *(float4*)(rast + 4 * o) = r;
        if (db) *(float4*)(db + 4 * o) = d;
    }
}

// rasterize backward, per pixel: d(u, v) at pixel (px, py) of triangle f -> the nine d(x), d(y), d(w) of its three clip positions (out) and the
// three vertex ids (vi).  DB: also the adjoint of the pixel derivatives db = (du/dX, du/dY, dv/dX, dv/dY) of resolve_pixel (gdb).  They are
// (dn{x,y}_0 - u dS{x,y}) / S and (dn{x,y}_1 - v dS{x,y}) / S in pixel units, with dnx_k = (Y_{k+1} - Y_{k+2}) q_k, dny_k = (X_{k+2} - X_{k+1}) q_k
// and dS{x,y} = sum_k dn{x,y}_k: gdb adds into gu / gv (the existing path), gives S a direct adjoint (gS), and lands on X, Y, q through
// dnx / dny directly.
template <bool DB>
__device__ __forceinline__ void raster_bwd_pixel_t(const float* __restrict__ posb, const int* __restrict__ tri, int f, int px, int py, int H, int W,
                                                   float gu, float gv, float4 gdb, float (&out)[9], int (&vi)[3]) {
    TriSetup t = load_tri(posb, tri, f);
    float fx = (px + 0.5f) * (2.0f / W) - 1.0f, fy = (py + 0.5f) * (2.0f / H) - 1.0f;
    float a[3];
    edge_fn(t, fx, fy, a);
    float n0 = a[0] * t.q[0], n1 = a[1] * t.q[1], n2 = a[2] * t.q[2];
    float S = n0 + n1 + n2, iS = 1.0f / S;
    float u = n0 * iS, v = n1 * iS;
    float ga[3], gq[3], gX[3] = {0.f, 0.f, 0.f}, gY[3] = {0.f, 0.f, 0.f};
    float gS = 0.f, gqd[3] = {0.f, 0.f, 0.f};
    if constexpr (DB) {
        const float dax[3] = {t.Y[1] - t.Y[2], t.Y[2] - t.Y[0], t.Y[0] - t.Y[1]};
        const float day[3] = {t.X[2] - t.X[1], t.X[0] - t.X[2], t.X[1] - t.X[0]};
        const float dSx = dax[0] * t.q[0] + dax[1] * t.q[1] + dax[2] * t.q[2], dSy = day[0] * t.q[0] + day[1] * t.q[1] + day[2] * t.q[2];
        const float h0 = gdb.x * (2.0f / W) * iS, h1 = gdb.y * (2.0f / H) * iS, h2 = gdb.z * (2.0f / W) * iS, h3 = gdb.w * (2.0f / H) * iS;
        gS = -(h0 * (dax[0] * t.q[0] - u * dSx) + h1 * (day[0] * t.q[0] - u * dSy) + h2 * (dax[1] * t.q[1] - v * dSx) +
               h3 * (day[1] * t.q[1] - v * dSy)) * iS;
        gu -= h0 * dSx + h1 * dSy;
        gv -= h2 * dSx + h3 * dSy;
        const float gSx = -(u * h0 + v * h2), gSy = -(u * h1 + v * h3);
        const float gdnx[3] = {h0 + gSx, h2 + gSx, gSx}, gdny[3] = {h1 + gSy, h3 + gSy, gSy};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            int j = (k + 1) % 3, l = (k + 2) % 3;
            gqd[k] = gdnx[k] * dax[k] + gdny[k] * day[k];
            const float gx = gdnx[k] * t.q[k], gy = gdny[k] * t.q[k];
            gY[j] += gx; gY[l] -= gx;               // dax_k = Y_j - Y_l
            gX[l] += gy; gX[j] -= gy;               // day_k = X_l - X_j
        }
    }
    float dotg = gu * u + gv * v;
    float gn[3] = {(gu - dotg) * iS, (gv - dotg) * iS, -dotg * iS};
    if constexpr (DB) {
#pragma unroll
        for (int k = 0; k < 3; ++k) gn[k] += gS;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) { ga[k] = gn[k] * t.q[k]; gq[k] = gn[k] * a[k]; }
    if constexpr (DB) {
#pragma unroll
        for (int k = 0; k < 3; ++k) gq[k] += gqd[k];
    }
    // a_i = (X_j - fx)(Y_k - fy) - (Y_j - fy)(X_k - fx), (j, k) = (i+1, i+2)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        int j = (k + 1) % 3, l = (k + 2) % 3;
        gX[j] += ga[k] * (t.Y[l] - fy);
        gY[l] += ga[k] * (t.X[j] - fx);
        gY[j] -= ga[k] * (t.X[l] - fx);
        gX[l] -= ga[k] * (t.Y[j] - fy);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        vi[k] = tri[3 * (size_t)f + k];
        float4 p = *(const float4*)(posb + 4 * (size_t)vi[k]);
        float q = t.q[k];
        float gqk = gq[k] + gX[k] * p.x + gY[k] * p.y;
        out[3 * k + 0] = gX[k] * q;
        out[3 * k + 1] = gY[k] * q;
        out[3 * k + 2] = -gqk * q * q;
    }
}
__device__ __forceinline__ void raster_bwd_pixel(const float* __restrict__ posb, const int* __restrict__ tri, int f, int px, int py, int H, int W,
                                                 float gu, float gv, float (&out)[9], int (&vi)[3]) {
    raster_bwd_pixel_t<false>(posb, tri, f, px, py, H, W, gu, gv, make_float4(0.f, 0.f, 0.f, 0.f), out, vi);
}

// rasterize backward: d(u, v) -> d(clip positions)
__global__ __launch_bounds__(256) void raster_bwd_kernel(const float* __restrict__ pos, int pos_bstride, const int* __restrict__ tri, int H, int W,
                                                         int nb, const float* __restrict__ rast, const float* __restrict__ g_rast,
                                                         float* __restrict__ d_pos /* same layout as pos */) {
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    size_t n = (size_t)nb * H * W;
    const int lane = threadIdx.x & 63;
    const bool inb = i < n;
    float4 r = inb ? *(const float4*)(rast + 4 * i) : make_float4(0.f, 0.f, 0.f, 0.f);
    const int id = (int)r.w;
    float4 g = (inb && id > 0) ? *(const float4*)(g_rast + 4 * i) : make_float4(0.f, 0.f, 0.f, 0.f);
    const float gu = g.x, gv = g.y;
    const bool live = id > 0 && !(gu == 0.f && gv == 0.f);
    if (__ballot(live) == 0ull) return;                 // wave-uniform
    const int b = inb ? (int)(i / ((size_t)H * W)) : 0;
    const D3hSeg sg = d3h_seg_runs(live ? id + (b << 24) : -1, lane);       // runs of lanes on the same triangle (see interp_bwd_kernel)
    float out[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};        // per vertex: d(x), d(y), d(w) of the clip position
    int vi[3] = {0, 0, 0};
    if (live) {
        int rem = (int)(i % ((size_t)H * W));
        raster_bwd_pixel(pos + (size_t)b * pos_bstride, tri, id - 1, rem % W, rem / W, H, W, gu, gv, out, vi);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float sx = d3h_seg_sum(out[3 * k + 0], lane, sg.start);
        float sy = d3h_seg_sum(out[3 * k + 1], lane, sg.start);
        float sw = d3h_seg_sum(out[3 * k + 2], lane, sg.start);
        if (sg.tail && live) {
            float* dp = d_pos + (size_t)b * pos_bstride + 4 * (size_t)vi[k];
            atomicAdd(dp + 0, sx);
            atomicAdd(dp + 1, sy);
            atomicAdd(dp + 3, sw);
        }
    }
}

// rasterize backward with the pixel derivatives: d(u, v) (g_rast, may be NULL) and d(du/dX, du/dY, dv/dX, dv/dY) (g_db, may be NULL) ->
// d(clip positions).  A pixel is live when either gradient is non-zero; the run reduction is raster_bwd_kernel's.
__global__ __launch_bounds__(256) void raster_bwd_db_kernel(const float* __restrict__ pos, int pos_bstride, const int* __restrict__ tri, int H, int W,
                                                            int nb, const float* __restrict__ rast, const float* __restrict__ g_rast,
                                                            const float* __restrict__ g_db, float* __restrict__ d_pos) {
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    size_t n = (size_t)nb * H * W;
    const int lane = threadIdx.x & 63;
    const bool inb = i < n;
    float4 r = inb ? *(const float4*)(rast + 4 * i) : make_float4(0.f, 0.f, 0.f, 0.f);
    const int id = (int)r.w;
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 g = (inb && id > 0 && g_rast) ? *(const float4*)(g_rast + 4 * i) : z4;
    const float4 gd = (inb && id > 0 && g_db) ? *(const float4*)(g_db + 4 * i) : z4;
    const bool live = id > 0 && !(g.x == 0.f && g.y == 0.f && gd.x == 0.f && gd.y == 0.f && gd.z == 0.f && gd.w == 0.f);
    if (__ballot(live) == 0ull) return;                 // wave-uniform
    const int b = inb ? (int)(i / ((size_t)H * W)) : 0;
    const D3hSeg sg = d3h_seg_runs(live ? id + (b << 24) : -1, lane);
    float out[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int vi[3] = {0, 0, 0};
    if (live) {
        int rem = (int)(i % ((size_t)H * W));
        raster_bwd_pixel_t<true>(pos + (size_t)b * pos_bstride, tri, id - 1, rem % W, rem / W, H, W, g.x, g.y, gd, out, vi);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float sx = d3h_seg_sum(out[3 * k + 0], lane, sg.start);
        float sy = d3h_seg_sum(out[3 * k + 1], lane, sg.start);
        float sw = d3h_seg_sum(out[3 * k + 2], lane, sg.start);
        if (sg.tail && live) {
            float* dp = d_pos + (size_t)b * pos_bstride + 4 * (size_t)vi[k];
            atomicAdd(dp + 0, sx);
            atomicAdd(dp + 1, sy);
            atomicAdd(dp + 3, sw);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// interpolate
// ------------------------------------------------------------------------------------------------
template <int MAXA>
__global__ __launch_bounds__(256) void interp_fwd_kernel(const float* __restrict__ attr, int attr_bstride, int na, const float* __restrict__ rast,
                                                         const int* __restrict__ tri, const float* __restrict__ db, size_t npix_total,
                                                         size_t npix_per_b, float* __restrict__ out, float* __restrict__ out_da) {
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= npix_total) return;
    float4 r = *(const float4*)(rast + 4 * i);
    int id = (int)r.w;
    float* o = out + i * na;
    if (id <= 0) {
        for (int c = 0; c < na; ++c) o[c] = 0.f;
        if (out_da) for (int c = 0; c < 2 * na; ++c) out_da[i * 2 * na + c] = 0.f;
        return;
    }
    int b = (int)(i / npix_per_b);
    const float* ab = attr + (size_t)b * attr_bstride;
    int f = id - 1;
    const float* a0 = ab + (size_t)tri[3 * (size_t)f] * na;
    const float* a1 = ab + (size_t)tri[3 * (size_t)f + 1] * na;
    const float* a2 = ab + (size_t)tri[3 * (size_t)f + 2] * na;
    float u = r.x, v = r.y, w = 1.0f - u - v;
    float4 d = make_float4(0.f, 0.f, 0.f, 0.f);
    if (out_da) d = *(const float4*)(db + 4 * i);
    for (int c = 0; c < na; ++c) {
        float x0 = a0[c], x1 = a1[c], x2 = a2[c];
        o[c] = u * x0 + v * x1 + w * x2;
        if (out_da) {
            float e0 = x0 - x2, e1 = x1 - x2;
            out_da[i * 2 * na + 2 * c + 0] = d.x * e0 + d.z * e1;
            out_da[i * 2 * na + 2 * c + 1] = d.y * e0 + d.w * e1;
        }
    }
}

__global__ __launch_bounds__(256) void interp_bwd_kernel(const float* __restrict__ attr, int attr_bstride, int na, const float* __restrict__ rast,
                                                         const int* __restrict__ tri, const float* __restrict__ g_out, size_t npix_total,
                                                         size_t npix_per_b, float* __restrict__ d_attr, float* __restrict__ d_rast) {
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool inb = i < npix_total;
    float4 r = inb ? *(const float4*)(rast + 4 * i) : make_float4(0.f, 0.f, 0.f, 0.f);
    const int id = (int)r.w;
    const bool hit = id > 0;
    if (__ballot(hit) == 0ull) {            // wave-uniform: nothing covered here
        if (d_rast && inb) *(float4*)(d_rast + 4 * i) = make_float4(0.f, 0.f, 0.f, 0.f);
        return;
    }
    const int b = inb ? (int)(i / npix_per_b) : 0;
    // runs of lanes on the same triangle of the same frame: one atomic per run and vertex instead of one per pixel (a triangle
    // covers ~10^2 pixels at 1024^2, i.e. ~10-20 consecutive pixels of a row)
    const D3hSeg sg = d3h_seg_runs(hit ? id + (b << 24) : -1, lane);
    float gu = 0.f, gv = 0.f;
    size_t i0 = 0, i1 = 0, i2 = 0;
    if (hit) {
        int f = id - 1;
        i0 = (size_t)tri[3 * (size_t)f] * na; i1 = (size_t)tri[3 * (size_t)f + 1] * na; i2 = (size_t)tri[3 * (size_t)f + 2] * na;
    }
    const float* ab = attr + (size_t)b * attr_bstride;
    float* db_ = d_attr ? d_attr + (size_t)b * attr_bstride : nullptr;
    const float u = r.x, v = r.y;
    const float* g = g_out + i * na;
    for (int c = 0; c < na; ++c) {
        float gc = hit ? g[c] : 0.f;
        if (db_) {      // (uniform) d(attr[v0]) += sum gc u, d(attr[v1]) += sum gc v, d(attr[v2]) += sum gc (1 - u - v)
            float s0 = d3h_seg_sum(gc * u, lane, sg.start);
            float s1 = d3h_seg_sum(gc * v, lane, sg.start);
            float s2 = d3h_seg_sum(gc * (1.0f - u - v), lane, sg.start);
            if (sg.tail && hit) {
                if (s0 != 0.f) atomicAdd(db_ + i0 + c, s0);
                if (s1 != 0.f) atomicAdd(db_ + i1 + c, s1);
                if (s2 != 0.f) atomicAdd(db_ + i2 + c, s2);
            }
        }
        if (hit && gc != 0.f) {
            float x2 = ab[i2 + c];
            gu = fmaf(gc, ab[i0 + c] - x2, gu);
            gv = fmaf(gc, ab[i1 + c] - x2, gv);
        }
    }
    if (d_rast && inb) *(float4*)(d_rast + 4 * i) = make_float4(gu, gv, 0.f, 0.f);
}

// interpolate with the pixel derivatives of a LIST of channels: out_da [npix][2 nidx], pair k = (d attr[idx[k]] / dX, d attr[idx[k]] / dY)
// (idx NULL: every channel in order, nidx = na -- interp_fwd_kernel's out_da)
__global__ __launch_bounds__(256) void interp_fwd_da_kernel(const float* __restrict__ attr, int attr_bstride, int na, const float* __restrict__ rast,
                                                            const int* __restrict__ tri, const float* __restrict__ db, const int* __restrict__ idx,
                                                            int nidx, size_t npix_total, size_t npix_per_b, float* __restrict__ out,
                                                            float* __restrict__ out_da) {
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= npix_total) return;
    float4 r = *(const float4*)(rast + 4 * i);
    int id = (int)r.w;
    float* o = out + i * na;
    float* od = out_da + i * 2 * nidx;
    if (id <= 0) {
        for (int c = 0; c < na; ++c) o[c] = 0.f;
        for (int c = 0; c < 2 * nidx; ++c) od[c] = 0.f;
        return;
    }
    int b = (int)(i / npix_per_b);
    const float* ab = attr + (size_t)b * attr_bstride;
    int f = id - 1;
    const float* a0 = ab + (size_t)tri[3 * (size_t)f] * na;
    const float* a1 = ab + (size_t)tri[3 * (size_t)f + 1] * na;
    const float* a2 = ab + (size_t)tri[3 * (size_t)f + 2] * na;
    float u = r.x, v = r.y, w = 1.0f - u - v;
    for (int c = 0; c < na; ++c) o[c] = u * a0[c] + v * a1[c] + w * a2[c];
    const float4 d = *(const float4*)(db + 4 * i);
    for (int k = 0; k < nidx; ++k) {
        const int c = idx ? idx[k] : k;
        float x2 = a2[c], e0 = a0[c] - x2, e1 = a1[c] - x2;
        od[2 * k + 0] = d.x * e0 + d.z * e1;
        od[2 * k + 1] = d.y * e0 + d.w * e1;
    }
}

// interpolate backward with the adjoint of the attribute pixel derivatives.  Per listed channel c = idx[k] (e0 = a0 - a2, e1 = a1 - a2 and
// (gX, gY) = g_da[2k], g_da[2k+1]): d a0 += gX db.x + gY db.y, d a1 += gX db.z + gY db.w, d a2 -= both, and d_db += (gX e0, gY e0, gX e1,
// gY e1).  g_out (may be NULL) goes as in interp_bwd_kernel; out_da does not depend on (u, v), so d_rast carries g_out's part only.  Runs of
// lanes on one triangle are reduced before the attribute atomics, as there.  idx NULL: every channel in order (nidx = na), folded into the
// g_out loop (one atomic per run, vertex and channel).
__global__ __launch_bounds__(256) void interp_bwd_da_kernel(const float* __restrict__ attr, int attr_bstride, int na, const float* __restrict__ rast,
                                                            const int* __restrict__ tri, const float* __restrict__ db, const int* __restrict__ idx,
                                                            int nidx, const float* __restrict__ g_out, const float* __restrict__ g_da,
                                                            size_t npix_total, size_t npix_per_b, float* __restrict__ d_attr,
                                                            float* __restrict__ d_rast, float* __restrict__ d_db) {
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool inb = i < npix_total;
    float4 r = inb ? *(const float4*)(rast + 4 * i) : make_float4(0.f, 0.f, 0.f, 0.f);
    const int id = (int)r.w;
    const bool hit = id > 0;
    if (__ballot(hit) == 0ull) {            // wave-uniform: nothing covered here
        if (d_rast && inb) *(float4*)(d_rast + 4 * i) = make_float4(0.f, 0.f, 0.f, 0.f);
        if (d_db && inb) *(float4*)(d_db + 4 * i) = make_float4(0.f, 0.f, 0.f, 0.f);
        return;
    }
    const int b = inb ? (int)(i / npix_per_b) : 0;
    const D3hSeg sg = d3h_seg_runs(hit ? id + (b << 24) : -1, lane);
    size_t i0 = 0, i1 = 0, i2 = 0;
    if (hit) {
        int f = id - 1;
        i0 = (size_t)tri[3 * (size_t)f] * na; i1 = (size_t)tri[3 * (size_t)f + 1] * na; i2 = (size_t)tri[3 * (size_t)f + 2] * na;
    }
    const float* ab = attr + (size_t)b * attr_bstride;
    float* dab = d_attr ? d_attr + (size_t)b * attr_bstride : nullptr;
    const float u = r.x, v = r.y;
    const float4 d = (hit && g_da) ? *(const float4*)(db + 4 * i) : make_float4(0.f, 0.f, 0.f, 0.f);
    float gu = 0.f, gv = 0.f;
    float4 gd = make_float4(0.f, 0.f, 0.f, 0.f);
    // per channel c: g_out part (when given), and the g_da part of channel c itself when the list is every channel (idx NULL)
    const bool fold = !idx && g_da;
    for (int c = 0; c < ((g_out || fold) ? na : 0); ++c) {
        const float gc = (hit && g_out) ? g_out[i * na + c] : 0.f;
        const float gX = (hit && fold) ? g_da[i * 2 * nidx + 2 * c] : 0.f, gY = (hit && fold) ? g_da[i * 2 * nidx + 2 * c + 1] : 0.f;
        const float p = gX * d.x + gY * d.y, q = gX * d.z + gY * d.w;
        if (dab) {
            float s0 = d3h_seg_sum(gc * u + p, lane, sg.start);
            float s1 = d3h_seg_sum(gc * v + q, lane, sg.start);
            float s2 = d3h_seg_sum(gc * (1.0f - u - v) - (p + q), lane, sg.start);
            if (sg.tail && hit) {
                if (s0 != 0.f) atomicAdd(dab + i0 + c, s0);
                if (s1 != 0.f) atomicAdd(dab + i1 + c, s1);
                if (s2 != 0.f) atomicAdd(dab + i2 + c, s2);
            }
        }
        if (hit && (gc != 0.f || gX != 0.f || gY != 0.f)) {
            float x2 = ab[i2 + c], e0 = ab[i0 + c] - x2, e1 = ab[i1 + c] - x2;
            gu = fmaf(gc, e0, gu);
            gv = fmaf(gc, e1, gv);
            gd.x = fmaf(gX, e0, gd.x); gd.y = fmaf(gY, e0, gd.y); gd.z = fmaf(gX, e1, gd.z); gd.w = fmaf(gY, e1, gd.w);
        }
    }
    // a list of channels (in any order, repeats allowed): one pass over the list
    for (int k = 0; k < ((idx && g_da) ? nidx : 0); ++k) {
        const int c = idx[k];
        const float gX = hit ? g_da[i * 2 * nidx + 2 * k] : 0.f, gY = hit ? g_da[i * 2 * nidx + 2 * k + 1] : 0.f;
        const float p = gX * d.x + gY * d.y, q = gX * d.z + gY * d.w;
        if (dab) {
            float s0 = d3h_seg_sum(p, lane, sg.start);
            float s1 = d3h_seg_sum(q, lane, sg.start);
            float s2 = d3h_seg_sum(-(p + q), lane, sg.start);
            if (sg.tail && hit) {
                if (s0 != 0.f) atomicAdd(dab + i0 + c, s0);
                if (s1 != 0.f) atomicAdd(dab + i1 + c, s1);
                if (s2 != 0.f) atomicAdd(dab + i2 + c, s2);
            }
        }
        if (hit && (gX != 0.f || gY != 0.f)) {
            float x2 = ab[i2 + c], e0 = ab[i0 + c] - x2, e1 = ab[i1 + c] - x2;
            gd.x = fmaf(gX, e0, gd.x); gd.y = fmaf(gY, e0, gd.y); gd.z = fmaf(gX, e1, gd.z); gd.w = fmaf(gY, e1, gd.w);
        }
    }
    if (d_rast && inb) *(float4*)(d_rast + 4 * i) = make_float4(gu, gv, 0.f, 0.f);
    if (d_db && inb) *(float4*)(d_db + 4 * i) = gd;
}

// ------------------------------------------------------------------------------------------------
// G-buffer: every interpolation of render_layer (render/render.py:257-267,283,328) in one pass over the raster
// ------------------------------------------------------------------------------------------------
// The reference calls dr.interpolate once per attribute (position, canonical position, normal, msdf with t_pos_idx; the face normal
// with an (f, f, f) index buffer) and derives the coverage mask from rast[..., 3] > 0.  Here the vertex attributes are the channel
// groups of one packed [nv][na] array, each group is written to its own contiguous image (its consumers -- the texture MLP, the
// composite pass -- read it without a strided copy, and groups nobody reads are not produced), the per-face attribute is a gather by
// triangle id, and the mask comes out of the same read of the raster.
constexpr int GBUF_GROUPS = 4;
struct GbufOut {
    float* out[GBUF_GROUPS];      // [npix][width[g]] or NULL (group skipped); group g covers channels [sum width[<g], ...) of attr
    int width[GBUF_GROUPS];
    float* face_out;              // [npix][fw] or NULL
    float* mask_out;              // [npix] or NULL: 1 where a triangle covers the pixel
};
struct GbufGrad {
    const float* g[GBUF_GROUPS];  // upstream gradients of the groups, NULL = zero
    int width[GBUF_GROUPS];
    const float* g_face;
};

__global__ __launch_bounds__(256) void gbuffer_fwd_kernel(const float* __restrict__ attr, int attr_bstride, int na,
                                                          const float* __restrict__ face_attr, int face_bstride, int fw,
                                                          const float* __restrict__ rast, const int* __restrict__ tri, size_t npix_total,
                                                          size_t npix_per_b, GbufOut o) {
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= npix_total) return;
    float4 r = *(const float4*)(rast + 4 * i);
    int id = (int)r.w;
    if (o.mask_out) o.mask_out[i] = id > 0 ? 1.f : 0.f;
    if (id <= 0) {
#pragma unroll
        for (int g = 0; g < GBUF_GROUPS; ++g)
            if (o.out[g]) for (int c = 0; c < o.width[g]; ++c) o.out[g][i * o.width[g] + c] = 0.f;
        if (o.face_out) for (int c = 0; c < fw; ++c) o.face_out[i * fw + c] = 0.f;
        return;
    }
    int b = (int)(i / npix_per_b);
    int f = id - 1;
    const float* ab = attr + (size_t)b * attr_bstride;
    const float* a0 = ab + (size_t)tri[3 * (size_t)f] * na;
    const float* a1 = ab + (size_t)tri[3 * (size_t)f + 1] * na;
    const float* a2 = ab + (size_t)tri[3 * (size_t)f + 2] * na;
    float u = r.x, v = r.y, w = 1.0f - u - v;
    int c0 = 0;
#pragma unroll
    for (int g = 0; g < GBUF_GROUPS; ++g) {
        if (o.out[g])
            for (int c = 0; c < o.width[g]; ++c) o.out[g][i * o.width[g] + c] = u * a0[c0 + c] + v * a1[c0 + c] + w * a2[c0 + c];
        c0 += o.width[g];
    }
    if (o.face_out) {
        const float* fa = face_attr + (size_t)b * face_bstride + (size_t)f * fw;
        // the reference interpolates three equal values: u x + v x + (1 - u - v) x, kept in that form (not bit-equal to x)
        for (int c = 0; c < fw; ++c) { float x = fa[c]; o.face_out[i * fw + c] = u * x + v * x + w * x; }
    }
}

// RAST: the rasteriser's backward in the same pass -- the barycentric gradient (gu, gv) of a covered pixel goes straight into d(clip
// positions) (raster_bwd_pixel; per-triangle runs reduced in the wave as everywhere here) instead of out to a [npix][4] image that
// raster_bwd_kernel reads back: 2 x 67 MB of traffic, one more read of the 67 MB raster and a launch per backward at 4 x 1024^2.
template <bool RAST>
__global__ __launch_bounds__(256) void gbuffer_bwd_kernel(const float* __restrict__ attr, int attr_bstride, int na, int face_bstride, int fw,
                                                          const float* __restrict__ rast, const int* __restrict__ tri, size_t npix_total,
                                                          size_t npix_per_b, GbufGrad gg, float* __restrict__ d_attr,
                                                          float* __restrict__ d_face, float* __restrict__ d_rast,
                                                          const float* __restrict__ pos, int pos_bstride, int H, int W, float* __restrict__ d_pos) {
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool inb = i < npix_total;
    float4 r = inb ? *(const float4*)(rast + 4 * i) : make_float4(0.f, 0.f, 0.f, 0.f);
    const int id = (int)r.w;
    const bool hit = id > 0;
    if (__ballot(hit) == 0ull) {            // wave-uniform: nothing covered here
        if (d_rast && inb) *(float4*)(d_rast + 4 * i) = make_float4(0.f, 0.f, 0.f, 0.f);
        return;
    }
    const int b = inb ? (int)(i / npix_per_b) : 0;
    const D3hSeg sg = d3h_seg_runs(hit ? id + (b << 24) : -1, lane);      // runs of lanes on one triangle: one atomic per run
    float gu = 0.f, gv = 0.f;
    size_t i0 = 0, i1 = 0, i2 = 0;
    const int f = hit ? id - 1 : 0;
    if (hit) { i0 = (size_t)tri[3 * (size_t)f] * na; i1 = (size_t)tri[3 * (size_t)f + 1] * na; i2 = (size_t)tri[3 * (size_t)f + 2] * na; }
    const float* ab = attr + (size_t)b * attr_bstride;
    float* db_ = d_attr ? d_attr + (size_t)b * attr_bstride : nullptr;
    const float u = r.x, v = r.y;
    int c0 = 0;
#pragma unroll
    for (int g = 0; g < GBUF_GROUPS; ++g) {
        const int wd = gg.width[g];
        if (gg.g[g]) {
            for (int c = 0; c < wd; ++c) {
                float gc = hit ? gg.g[g][i * wd + c] : 0.f;
                const int ch = c0 + c;
                if (db_) {
                    float s0 = d3h_seg_sum(gc * u, lane, sg.start);
                    float s1 = d3h_seg_sum(gc * v, lane, sg.start);
                    float s2 = d3h_seg_sum(gc * (1.0f - u - v), lane, sg.start);
                    if (sg.tail && hit) {
                        if (s0 != 0.f) atomicAdd(db_ + i0 + ch, s0);
                        if (s1 != 0.f) atomicAdd(db_ + i1 + ch, s1);
                        if (s2 != 0.f) atomicAdd(db_ + i2 + ch, s2);
                    }
                }
                if (hit && gc != 0.f) {
                    float x2 = ab[i2 + ch];
                    gu = fmaf(gc, ab[i0 + ch] - x2, gu);
                    gv = fmaf(gc, ab[i1 + ch] - x2, gv);
                }
            }
        }
        c0 += wd;
    }
    if (gg.g_face && d_face) {              // u + v + (1 - u - v) of the gradient lands on the one face row; no barycentric gradient
        float* df = d_face + (size_t)b * face_bstride + (size_t)f * fw;
        for (int c = 0; c < fw; ++c) {
            float gc = hit ? gg.g_face[i * fw + c] : 0.f;
            float s = d3h_seg_sum(gc * u, lane, sg.start) + d3h_seg_sum(gc * v, lane, sg.start) + d3h_seg_sum(gc * (1.0f - u - v), lane, sg.start);
            if (sg.tail && hit && s != 0.f) atomicAdd(df + c, s);
        }
    }
    if (d_rast && inb) *(float4*)(d_rast + 4 * i) = make_float4(gu, gv, 0.f, 0.f);
    if (RAST) {
        const bool live = hit && !(gu == 0.f && gv == 0.f);
        if (__ballot(live) == 0ull) return;             // wave-uniform
        float out[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        int vi[3];
        if (live) {
            const int rem = (int)(i % npix_per_b);
            raster_bwd_pixel(pos + (size_t)b * pos_bstride, tri, f, rem % W, rem / W, H, W, gu, gv, out, vi);
        }
        // (the runs are those of the covered lanes, every lane of a run on triangle f: lanes without a barycentric gradient add zeros)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float sx = d3h_seg_sum(out[3 * k + 0], lane, sg.start);
            const float sy = d3h_seg_sum(out[3 * k + 1], lane, sg.start);
            const float sw = d3h_seg_sum(out[3 * k + 2], lane, sg.start);
            if (sg.tail && hit && (sx != 0.f || sy != 0.f || sw != 0.f)) {
                float* dp = d_pos + (size_t)b * pos_bstride + 4 * (size_t)tri[3 * (size_t)f + k];
                atomicAdd(dp + 0, sx);
                atomicAdd(dp + 1, sy);
                atomicAdd(dp + 3, sw);
            }
        }
    }
}

// ---- the same backward with the sums taken per workgroup in LDS ---------------------------------------------------------------------
// gbuffer_bwd_kernel above is bound by memory-side float atomics: a workgroup owns 256 pixels of ONE row, a triangle of ~30 pixels spans
// 5-6 rows, so every triangle is cut into many runs and each run tail issues, per vertex and channel, a single-lane atomic (a 64-B request
// for 4 useful bytes).  The destinations are few (vertices x (na + 3) floats), so here a workgroup owns a 2-D TW x TH tile of one frame, the
// run tails add into an LDS table keyed by vertex index (one row of na d(attr) floats + d(pos) x, y, w when RAST per slot; a second small
// table keyed by face id for d(face)), and after a barrier consecutive lanes flush consecutive floats of a slot's row: one atomic
// wave-instruction covers whole rows.  A key that finds no slot within GBL_PROBES steps (table full) sends its contribution straight to
// global memory with the atomics of the kernel above: no spin-wait anywhere, every path ends for any input.
constexpr int GBL_VCAP = 256, GBL_VPOOL = 4096;     // vertex table: slots (power of two), floats (256 slots of up to 16 floats)
constexpr int GBL_FCAP = 256, GBL_FPOOL = 1024;     // face table
constexpr int GBL_PROBES = 8;
constexpr int GBL_SLOTS = 64;                       // slots in use by default (a 16 x 16 tile of the flagship frames sees ~25 vertices)

// slot of `key` (>= 0) in an open-addressing table of `cap` (power of two, or 0 = no table) LDS keys initialised to -1; -1 = no slot found
__device__ __forceinline__ int gbl_claim(int* keys, int cap, int key) {
    if (cap == 0) return -1;
    int s = (int)(((unsigned)key * 0x9E3779B1u) >> 16) & (cap - 1);
    for (int p = 0; p < GBL_PROBES && p < cap; ++p) {
        const int old = atomicCAS(&keys[s], -1, key);
        if (old == -1 || old == key) return s;
        s = (s + 1) & (cap - 1);
    }
    return -1;
}

template <bool RAST, int TW, int TH>
__global__ __launch_bounds__(256) void gbuffer_bwd_tile_kernel(const float* __restrict__ attr, int attr_bstride, int na, int face_bstride, int fw,
                                                               const float* __restrict__ rast, const int* __restrict__ tri, GbufGrad gg,
                                                               float* __restrict__ d_attr, float* __restrict__ d_face, float* __restrict__ d_rast,
                                                               const float* __restrict__ pos, int pos_bstride, int H, int W,
                                                               float* __restrict__ d_pos, int vcap, int fcap) {
    static_assert((TW * TH) % 256 == 0 && TW <= 256 && 256 % TW == 0, "a pass of the workgroup covers whole tile rows");
    __shared__ __attribute__((aligned(16))) float vval[GBL_VPOOL];
    __shared__ __attribute__((aligned(16))) float fval[GBL_FPOOL];
    __shared__ int vkey[GBL_VCAP];
    __shared__ int fkey[GBL_FCAP];
    const int tid = threadIdx.x, lane = tid & 63;
    const int b = blockIdx.z;
    const int na_v = d_attr ? na : 0;                       // floats of a vertex slot: d(attr) row, then d(pos) x, y, w
    const int vstride = na_v + (RAST ? 3 : 0);
    const bool want_face = gg.g_face && d_face;
    // Most tiles of a frame see no triangle: they leave after a vote (and their zeros of d_rast), without touching the tables.
    __shared__ int s_any;
    if (tid == 0) s_any = 0;
    __syncthreads();
    {
        bool any = false;
        for (int pass = 0; pass < TW * TH / 256; ++pass) {
            const int lp = pass * 256 + tid;
            const int px = blockIdx.x * TW + lp % TW, py = blockIdx.y * TH + lp / TW;
            if (px < W && py < H) any = any || rast[4 * (((size_t)b * H + py) * W + px) + 3] > 0.f;
        }
        if (any) s_any = 1;
    }
    __syncthreads();
    if (!s_any) {
        if (d_rast) {
            for (int pass = 0; pass < TW * TH / 256; ++pass) {
                const int lp = pass * 256 + tid;
                const int px = blockIdx.x * TW + lp % TW, py = blockIdx.y * TH + lp / TW;
                if (px < W && py < H) *(float4*)(d_rast + 4 * (((size_t)b * H + py) * W + px)) = make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
        return;
    }
    // (the pools are multiples of four floats: the rounded-up tail of the last float4 stays inside them)
    for (int k = tid; k < vcap; k += 256) vkey[k] = -1;
    for (int k = 4 * tid; k < vcap * vstride; k += 1024) *(float4*)&vval[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (want_face) {
        for (int k = tid; k < fcap; k += 256) fkey[k] = -1;
        for (int k = 4 * tid; k < fcap * fw; k += 1024) *(float4*)&fval[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    __syncthreads();
    const float* ab = attr + (size_t)b * attr_bstride;
    float* db_ = d_attr ? d_attr + (size_t)b * attr_bstride : nullptr;
    float* dfb = want_face ? d_face + (size_t)b * face_bstride : nullptr;
    float* dpb = RAST ? d_pos + (size_t)b * pos_bstride : nullptr;
#pragma unroll 1
    for (int pass = 0; pass < TW * TH / 256; ++pass) {
        const int lp = pass * 256 + tid;
        const int px = blockIdx.x * TW + lp % TW, py = blockIdx.y * TH + lp / TW;
        const bool inb = px < W && py < H;
        const size_t i = ((size_t)b * H + (inb ? py : 0)) * W + (inb ? px : 0);
        float4 r = inb ? *(const float4*)(rast + 4 * i) : make_float4(0.f, 0.f, 0.f, 0.f);
        const int id = (int)r.w;
        const bool hit = id > 0;
        if (__ballot(hit) == 0ull) {            // wave-uniform: nothing covered here
            if (d_rast && inb) *(float4*)(d_rast + 4 * i) = make_float4(0.f, 0.f, 0.f, 0.f);
            continue;
        }
        const D3hSeg sg = d3h_seg_runs(hit ? id : -1, lane);               // runs of lanes on one triangle (the tile is in one frame)
        const bool tail = sg.tail && hit;
        float gu = 0.f, gv = 0.f;
        const int f = hit ? id - 1 : 0;
        int vi[3] = {0, 0, 0};
        if (hit) { vi[0] = tri[3 * (size_t)f]; vi[1] = tri[3 * (size_t)f + 1]; vi[2] = tri[3 * (size_t)f + 2]; }
        const size_t i0 = (size_t)vi[0] * na, i1 = (size_t)vi[1] * na, i2 = (size_t)vi[2] * na;
        int sl[3] = {-1, -1, -1};                                           // the run tail's slots of its three vertices
        if (tail && vstride > 0) {
#pragma unroll
            for (int k = 0; k < 3; ++k) sl[k] = gbl_claim(vkey, vcap, vi[k]);
        }
        const float u = r.x, v = r.y;
        int c0 = 0;
#pragma unroll
        for (int g = 0; g < GBUF_GROUPS; ++g) {
            const int wd = gg.width[g];
            if (gg.g[g]) {
                for (int c = 0; c < wd; ++c) {
                    float gc = hit ? gg.g[g][i * wd + c] : 0.f;
                    const int ch = c0 + c;
                    if (db_) {
                        float s0 = d3h_seg_sum(gc * u, lane, sg.start);
                        float s1 = d3h_seg_sum(gc * v, lane, sg.start);
                        float s2 = d3h_seg_sum(gc * (1.0f - u - v), lane, sg.start);
                        if (tail) {
                            if (s0 != 0.f) { if (sl[0] >= 0) atomicAdd(&vval[sl[0] * vstride + ch], s0); else atomicAdd(db_ + i0 + ch, s0); }
                            if (s1 != 0.f) { if (sl[1] >= 0) atomicAdd(&vval[sl[1] * vstride + ch], s1); else atomicAdd(db_ + i1 + ch, s1); }
                            if (s2 != 0.f) { if (sl[2] >= 0) atomicAdd(&vval[sl[2] * vstride + ch], s2); else atomicAdd(db_ + i2 + ch, s2); }
                        }
                    }
                    if (hit && gc != 0.f) {
                        float x2 = ab[i2 + ch];
                        gu = fmaf(gc, ab[i0 + ch] - x2, gu);
                        gv = fmaf(gc, ab[i1 + ch] - x2, gv);
                    }
                }
            }
            c0 += wd;
        }
        if (want_face) {                        // u + v + (1 - u - v) of the gradient lands on the one face row; no barycentric gradient
            const int sf = tail ? gbl_claim(fkey, fcap, f) : -1;
            for (int c = 0; c < fw; ++c) {
                float gc = hit ? gg.g_face[i * fw + c] : 0.f;
                float s = d3h_seg_sum(gc * u, lane, sg.start) + d3h_seg_sum(gc * v, lane, sg.start) + d3h_seg_sum(gc * (1.0f - u - v), lane, sg.start);
                if (tail && s != 0.f) { if (sf >= 0) atomicAdd(&fval[sf * fw + c], s); else atomicAdd(dfb + (size_t)f * fw + c, s); }
            }
        }
        if (d_rast && inb) *(float4*)(d_rast + 4 * i) = make_float4(gu, gv, 0.f, 0.f);
        if (RAST) {
            const bool live = hit && !(gu == 0.f && gv == 0.f);
            if (__ballot(live) == 0ull) continue;           // wave-uniform
            float out[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            int vj[3];
            if (live) raster_bwd_pixel(pos + (size_t)b * pos_bstride, tri, f, px, py, H, W, gu, gv, out, vj);
            // (the runs are those of the covered lanes, every lane of a run on triangle f: lanes without a barycentric gradient add zeros)
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float sx = d3h_seg_sum(out[3 * k + 0], lane, sg.start);
                const float sy = d3h_seg_sum(out[3 * k + 1], lane, sg.start);
                const float sw = d3h_seg_sum(out[3 * k + 2], lane, sg.start);
                if (tail && (sx != 0.f || sy != 0.f || sw != 0.f)) {
                    if (sl[k] >= 0) {
                        float* dv = &vval[sl[k] * vstride + na_v];
                        atomicAdd(dv + 0, sx);
                        atomicAdd(dv + 1, sy);
                        atomicAdd(dv + 2, sw);
                    } else {
                        float* dp = dpb + 4 * (size_t)vi[k];
                        atomicAdd(dp + 0, sx);
                        atomicAdd(dp + 1, sy);
                        atomicAdd(dp + 3, sw);
                    }
                }
            }
        }
    }
    __syncthreads();
    // flush: consecutive lanes take consecutive floats of a slot's row; zero entries (and empty slots, which are all zero) are skipped
    // (16 lanes per slot: unused slots cost one key read)
    for (int k = tid; k < vcap * 16; k += 256) {
        const int slot = k >> 4, key = vkey[slot];
        if (key < 0) continue;
        for (int c = k & 15; c < vstride; c += 16) {
            const float s = vval[slot * vstride + c];
            if (s == 0.f) continue;
            if (c < na_v) atomicAdd(db_ + (size_t)key * na + c, s);
            else if (RAST) atomicAdd(dpb + 4 * (size_t)key + (c - na_v == 2 ? 3 : c - na_v), s);
        }
    }
    if (want_face) {
        for (int k = tid; k < fcap * 4; k += 256) {
            const int slot = k >> 2, key = fkey[slot];
            if (key < 0) continue;
            for (int c = k & 3; c < fw; c += 4) {
                const float s = fval[slot * fw + c];
                if (s != 0.f) atomicAdd(dfb + (size_t)key * fw + c, s);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// antialias
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned hash64(unsigned long long k) {
    k ^= k >> 33; k *= 0xff51afd7ed558ccdull; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull; k ^= k >> 33;
    return (unsigned)k;
}

// edge -> opposite vertices of (up to) two adjacent triangles
__global__ void aa_hash_build_kernel(const int* __restrict__ tri, int nf, unsigned long long* __restrict__ keys, int* __restrict__ vals, unsigned mask) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 3 * nf) return;
    int f = i / 3, e = i % 3;
    int va = tri[3 * (size_t)f + e], vb = tri[3 * (size_t)f + (e + 1) % 3], vo = tri[3 * (size_t)f + (e + 2) % 3];
    if (va == vb) return;
    unsigned long long key = ((unsigned long long)(unsigned)min(va, vb) << 32) | (unsigned)max(va, vb);
    unsigned slot = hash64(key) & mask;
    for (unsigned probe = 0; probe <= mask; ++probe) {
        unsigned long long prev = atomicCAS(&keys[slot], ~0ull, key);
        if (prev == ~0ull || prev == key) {
            if (atomicCAS(&vals[2 * slot], -1, vo) != -1) atomicCAS(&vals[2 * slot + 1], -1, vo);
            return;
        }
        slot = (slot + 1) & mask;
    }
}

__device__ __forceinline__ int hash_other(const unsigned long long* __restrict__ keys, const int* __restrict__ vals, unsigned mask, int va, int vb,
                                          int vo) {
    unsigned long long key = ((unsigned long long)(unsigned)min(va, vb) << 32) | (unsigned)max(va, vb);
    unsigned slot = hash64(key) & mask;
    for (unsigned probe = 0; probe <= mask; ++probe) {
        unsigned long long k = keys[slot];
        if (k == key) {
            int o0 = vals[2 * slot], o1 = vals[2 * slot + 1];
            if (o1 == -1) return -1;            // boundary edge
            return (o0 == vo) ? o1 : o0;
        }
        if (k == ~0ull) return -1;
        slot = (slot + 1) & mask;
    }
    return -1;
}

struct AAHit {
    int pi, po;          // flat pixel indices (within the batch item) of the inner (foreground) and outer pixel
    int va, vb;          // vertex ids of the silhouette edge
    float d;             // crossing position in [0, 1] from the inner pixel centre towards the outer one
    bool ok;
};

// Per (frame, triangle): bit e set <=> edge e (vertices e, e+1) is a SILHOUETTE edge in that frame: it has no second triangle, or the
// opposite vertex of its neighbour lies on the same side of it in screen space as the triangle's own (a fold), or that vertex is
// behind the camera.  This is the part of the pair analysis that does not depend on the pixel, so it is evaluated once per render
// (~10^4 triangles x 3 hash probes) instead of once per pixel pair: almost every pair of pixels with different ids straddles an
// INTERIOR edge, and with the flags at hand such a pair is dismissed after one byte load, before any vertex is fetched.
__global__ void aa_edge_flags_kernel(const float* __restrict__ pos, int pos_bstride, const int* __restrict__ tri, int nf, int nb,
                                     const unsigned long long* __restrict__ keys, const int* __restrict__ vals, unsigned mask, int H, int W,
                                     unsigned char* __restrict__ flags) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nf * nb) return;
    const int b = i / nf, f = i % nf;
    const float* posb = pos + (size_t)b * pos_bstride;
    int vid[3];
    float sx[3], sy[3];
    bool front = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        vid[k] = tri[3 * (size_t)f + k];
        float4 p = *(const float4*)(posb + 4 * (size_t)vid[k]);
        front = front && (p.w > 1e-8f);
        float q = 1.0f / p.w;
        sx[k] = (p.x * q * 0.5f + 0.5f) * W;
        sy[k] = (p.y * q * 0.5f + 0.5f) * H;
    }
    if (!front) { flags[i] = 0; return; }        // a triangle that crosses the camera plane has no screen-space silhouette edges: not blended
    unsigned fl = 0;
#pragma unroll
    for (int e = 0; e < 3; ++e) {
        const int ia = e, ib = (e + 1) % 3, io = (e + 2) % 3;
        const float xa = sx[ia], ya = sy[ia], xb = sx[ib], yb = sy[ib];
        bool sil = true;
        const int other = hash_other(keys, vals, mask, vid[ia], vid[ib], vid[io]);
        if (other >= 0) {
            float4 p = *(const float4*)(posb + 4 * (size_t)other);
            if (p.w > 1e-8f) {
                float q = 1.0f / p.w;
                float ox = (p.x * q * 0.5f + 0.5f) * W, oy = (p.y * q * 0.5f + 0.5f) * H;
                float side_c = (xb - xa) * (sy[io] - ya) - (yb - ya) * (sx[io] - xa);
                float side_o = (xb - xa) * (oy - ya) - (yb - ya) * (ox - xa);
                if (side_c * side_o < 0.f) sil = false;     // opposite sides: interior edge
            }
        }
        if (sil) fl |= 1u << e;
    }
    flags[i] = (unsigned char)fl;
}

// analyse the pixel pair (x, y) -> (x + dx, y + dy); flags_b: the silhouette-edge bits of this frame's triangles
__device__ __forceinline__ AAHit aa_analyse(const float* __restrict__ rast_b, const float* __restrict__ posb, const int* __restrict__ tri,
                                            const unsigned char* __restrict__ flags_b, int x, int y, int dirx, int H, int W) {
    AAHit hit;
    hit.ok = false;
    hit.pi = hit.po = hit.va = hit.vb = 0;
    hit.d = 0.f;
    int x1 = x + dirx, y1 = y + (1 - dirx);
    if (x1 >= W || y1 >= H) return hit;
    int p0 = y * W + x, p1 = y1 * W + x1;
    float4 r0 = *(const float4*)(rast_b + 4 * (size_t)p0), r1 = *(const float4*)(rast_b + 4 * (size_t)p1);
    int t0 = (int)r0.w, t1 = (int)r1.w;
    if (t0 == t1) return hit;
    bool first = (t1 == 0) || (t0 != 0 && r0.z < r1.z);     // which pixel holds the nearer surface
    int tf = first ? t0 : t1;
    int f = tf - 1;
    const unsigned fl = flags_b[f];
    if (!fl) return hit;                                     // the nearer triangle has no silhouette edge: nothing to blend
    hit.pi = first ? p0 : p1;
    hit.po = first ? p1 : p0;
    float cxi = (first ? x : x1) + 0.5f, cyi = (first ? y : y1) + 0.5f;
    float cxo = (first ? x1 : x) + 0.5f, cyo = (first ? y1 : y) + 0.5f;
    int vid[3];
    float sx[3], sy[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        vid[k] = tri[3 * (size_t)f + k];
        float4 p = *(const float4*)(posb + 4 * (size_t)vid[k]);
        float q = 1.0f / p.w;
        sx[k] = (p.x * q * 0.5f + 0.5f) * W;
        sy[k] = (p.y * q * 0.5f + 0.5f) * H;
    }
#pragma unroll
    for (int e = 0; e < 3; ++e) {
        if (!((fl >> e) & 1u)) continue;                     // interior edge
        int ia = e, ib = (e + 1) % 3;
        float xa = sx[ia], ya = sy[ia], xb = sx[ib], yb = sy[ib];
        // crossing of the edge with the segment between the two pixel centres
        float d;
        if (dirx) {
            float lo = fminf(ya, yb), hi = fmaxf(ya, yb);
            if (!(cyi >= lo && cyi <= hi) || ya == yb) continue;
            if (fabsf(yb - ya) < fabsf(xb - xa)) continue;      // horizontal pairs only see edges closer to vertical: |d xe / d y| <= 1
            float tt = (cyi - ya) / (yb - ya);
            float xe = xa + tt * (xb - xa);
            d = (xe - cxi) / (cxo - cxi);
        } else {
            float lo = fminf(xa, xb), hi = fmaxf(xa, xb);
            if (!(cxi >= lo && cxi <= hi) || xa == xb) continue;
            if (fabsf(xb - xa) < fabsf(yb - ya)) continue;      // vertical pairs only see edges closer to horizontal
            float tt = (cxi - xa) / (xb - xa);
            float ye = ya + tt * (yb - ya);
            d = (ye - cyi) / (cyo - cyi);
        }
        if (!(d >= 0.f && d <= 1.f)) continue;
        hit.ok = true;
        hit.va = vid[ia]; hit.vb = vid[ib];
        hit.d = d;
        return hit;
    }
    return hit;
}

// The four pixel pairs a pixel takes part in: the two it owns (right, down) and the two owned by its left / upper neighbour.
// `self_is_dst` / `other`: whether this pixel is the blended one of the pair, and the flat index of the pair's other pixel.
struct AAPair { AAHit h; bool ok; bool self_is_dst; int other; float wgt; };
__device__ __forceinline__ AAPair aa_pair(const float* __restrict__ rast_b, const float* __restrict__ posb, const int* __restrict__ tri,
                                          const unsigned char* __restrict__ flags_b, int x, int y, int k, int H, int W) {
    // k: 0 = (x, y)-(x+1, y), 1 = (x, y)-(x, y+1), 2 = (x-1, y)-(x, y), 3 = (x, y-1)-(x, y)
    AAPair r;
    r.ok = false;
    const int ox = (k == 2) ? x - 1 : x, oy = (k == 3) ? y - 1 : y;          // owner of the pair
    const int dirx = (k == 0 || k == 2) ? 1 : 0;
    if (ox < 0 || oy < 0) return r;
    r.h = aa_analyse(rast_b, posb, tri, flags_b, ox, oy, dirx, H, W);
    if (!r.h.ok) return r;
    const float alpha = r.h.d - 0.5f;
    const int dst = (alpha >= 0.f) ? r.h.po : r.h.pi;
    const int src = (alpha >= 0.f) ? r.h.pi : r.h.po;
    const int self = y * W + x;
    r.ok = true;
    r.self_is_dst = (dst == self);
    r.other = r.self_is_dst ? src : dst;
    r.wgt = fabsf(alpha);
    return r;
}

// Does pixel (x, y) differ in triangle id from one of its four neighbours?  Called by ALL lanes of a wave (i = flat pixel index of the lane,
// valid = i < n): the lane's own id comes from one coalesced 16-byte load, the left / right ids from the neighbouring lanes (pixels of a
// row are consecutive lanes) except at the two ends of the wave; only the rows above and below cost a strided load each.
__device__ __forceinline__ bool aa_on_discontinuity(const float* __restrict__ rast, size_t i, bool valid, int x, int y, int H, int W) {
    const float t = valid ? ((const float4*)rast)[i].w : -1.f;
    const int lane = threadIdx.x & 63;
    float tl = __shfl_up(t, 1), tr = __shfl_down(t, 1);
    if (!valid) return false;
    if (lane == 0 && x > 0) tl = rast[4 * (i - 1) + 3];
    if (lane == 63 && x + 1 < W) tr = rast[4 * (i + 1) + 3];
    bool diff = false;
    if (x + 1 < W) diff |= tr != t;
    if (x > 0) diff |= tl != t;
    if (y + 1 < H) diff |= rast[4 * (i + W) + 3] != t;
    if (y > 0) diff |= rast[4 * (i - W) + 3] != t;
    return diff;
}

// Pixels per workgroup of the two antialias kernels: AA_TILES sub-tiles of 256 consecutive pixels.  With one sub-tile per workgroup a thread
// had ~2 float4 of the copy in flight and the kernels sat at 90 % SQ_WAIT_ANY (profiles/r3_pmc_image_space_kernels.txt: 3.0 / 3.5 TB/s).
// Measured at 4 x 1024^2 x 9 channels, serialised (tools/dbg/ab_aa.sh): 1 / 2 / 4 / 8 sub-tiles: forward 124 / 117 / 117 / 140 us, backward
// 149 / 134 / 136 / 170 us.  What is left is the raster: every pixel reads its own 16-byte entry and the ids of the rows above and below
// (4 useful bytes per 16 fetched), i.e. the 67 MB raster three times next to 2 x 151 MB of image.
#ifndef D3H_AA_TILES
#define D3H_AA_TILES 2
#endif
constexpr int AA_TILES = D3H_AA_TILES;
constexpr int AA_WG_PIX = 256 * AA_TILES;

// ---- what the six antialias kernels share ---------------------------------------------------------------------------------------------------
// The three pairs of kernels differ in the pre-antialias image only: stored (aa_fwd / aa_bwd), composited on the fly from the layer buffers
// (aa_composite_*), blended on the fly over `under` (layer_composite_*).  Each describes it as a functor `Pre`:
//     Pre::At             what the image at a pixel depends on besides the channel (its index, coverage, weight)
//     pre.at(p)           that, for pixel p of the frame
//     pre.channels(fn)    calls fn(ch, val) for every channel ch of a row in turn; val(at) is the value of that channel at such a pixel
// and everything else of phase 2 is written once, below.

// A pixel of phase 2: its frame, the frame's slices of the inputs, and the four pairs it takes part in.
struct AAPixel {
    int b, x, y, self;                        // frame, column, row, y * W + x
    size_t gb0;                               // global pixel index of the frame's first pixel
    const float* rast_b;
    const float* posb;
    const unsigned char* flags_b;
    AAPair pr[4];
};

// Set up pixel i (flat index over all frames: rows of consecutive frames are consecutive in memory).  Called by ALL lanes of a wave, in a loop
// whose trip count is workgroup-uniform (aa_on_discontinuity is a wave-level operation); false: nothing to do for this pixel.  FWD: only the
// pairs that blend INTO this pixel with a non-zero weight stay `ok` (the forward kernels rewrite their own pixel); otherwise all pairs do.
template <bool FWD>
__device__ __forceinline__ bool aa_pixel(AAPixel& px, size_t i, size_t n, const float* __restrict__ rast, const float* __restrict__ pos, int pos_bstride,
                                         const int* __restrict__ tri, const unsigned char* __restrict__ flags, int nf, int H, int W) {
    const size_t hw = (size_t)H * W;
    int b = 0, x = 0, y = 0;
    if (i < n) {
        b = (int)(i / hw);
        const int rem = (int)(i % hw);
        y = rem / W; x = rem % W;
    }
    if (!aa_on_discontinuity(rast, i, i < n, x, y, H, W)) return false;
    px.b = b; px.x = x; px.y = y; px.self = y * W + x;
    px.gb0 = (size_t)b * hw;
    px.rast_b = rast + 4 * px.gb0;
    px.posb = pos + (size_t)b * pos_bstride;
    px.flags_b = flags + (size_t)b * nf;
    bool any = false;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        px.pr[k] = aa_pair(px.rast_b, px.posb, tri, px.flags_b, x, y, k, H, W);
        if (FWD) px.pr[k].ok = px.pr[k].ok && px.pr[k].self_is_dst && px.pr[k].wgt != 0.f;
        any |= px.pr[k].ok;
    }
    return any;
}

// Forward, a pixel set up with FWD: orow[ch] = pre[self] + sum over its pairs of w (pre[other] - pre[self]), orow = the pixel's row of `out`.
template <class Pre>
__device__ __forceinline__ void aa_blend(const AAPixel& px, const Pre& pre, float* __restrict__ orow) {
    const typename Pre::At self = pre.at(px.self);
    typename Pre::At oth[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) oth[k] = px.pr[k].ok ? pre.at(px.pr[k].other) : typename Pre::At{};
    pre.channels([&](int ch, auto val) {
        const float base = val(self);
        float v = base;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (px.pr[k].ok) v += px.pr[k].wgt * (val(oth[k]) - base);
        orow[ch] = v;
    });
}

// Backward: does any pair move this pixel's pre-antialias gradient away from g_out[self]?
__device__ __forceinline__ bool aa_touched(const AAPixel& px) {
    bool touch = false;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (px.pr[k].ok && px.pr[k].wgt != 0.f) touch = true;
    return touch;
}

// Backward: the gradient of channel ch of this pixel's pre-antialias row, gathered (gb: the frame's g_out, C floats per pixel):
// g[self] (1 - sum of the weights of the pairs that blend INTO self) + sum over the pairs that blend self into their other pixel q of w g[q]
__device__ __forceinline__ float aa_gather(const AAPixel& px, const float* __restrict__ gb, int C, int ch) {
    const float gs = gb[(size_t)px.self * C + ch];
    float v = gs;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (!px.pr[k].ok || px.pr[k].wgt == 0.f) continue;
        if (px.pr[k].self_is_dst) v -= px.pr[k].wgt * gs;                                  // out[self] = ... - w pre[self]
        else v += px.pr[k].wgt * gb[(size_t)px.pr[k].other * C + ch];                      // out[other] = ... + w pre[self]
    }
    return v;
}

// Backward: the position gradient of one pair, h its analysis, gd = d loss / d d (d = h.d, the crossing in units of the pixel distance);
// dpb: the frame's slice of d_pos (float atomics).
__device__ __forceinline__ void aa_pos_grad(const AAHit& h, int dirx, float gd, const float* __restrict__ posb, float* __restrict__ dpb, int H, int W) {
    // d = (e - c_i) / (c_o - c_i) with c_o - c_i = +-1 along the pair axis; e = crossing coordinate
    float px_i = (float)(h.pi % W) + 0.5f, py_i = (float)(h.pi / W) + 0.5f;
    float px_o = (float)(h.po % W) + 0.5f, py_o = (float)(h.po / W) + 0.5f;
    // edge end points in pixel coordinates, recomputed from the clip-space vertices
    int vv[2] = {h.va, h.vb};
    float4 pc[2];
    float qv[2], ex[2], ey[2];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
        pc[kk] = *(const float4*)(posb + 4 * (size_t)vv[kk]);
        qv[kk] = 1.0f / pc[kk].w;
        ex[kk] = (pc[kk].x * qv[kk] * 0.5f + 0.5f) * W;
        ey[kk] = (pc[kk].y * qv[kk] * 0.5f + 0.5f) * H;
    }
    float gsx[2], gsy[2];
    if (dirx) {
        float ge = gd / (px_o - px_i);
        float dy = ey[1] - ey[0];
        float tt = (py_i - ey[0]) / dy;
        // xe = xa + tt (xb - xa), tt = (cy - ya)/(yb - ya)
        float gtt = ge * (ex[1] - ex[0]);
        gsx[0] = ge * (1.f - tt); gsx[1] = ge * tt;
        gsy[0] = gtt * (tt - 1.f) / dy;      // d tt/d ya = (tt - 1)/dy
        gsy[1] = -gtt * tt / dy;             // d tt/d yb = -tt/dy
    } else {
        float ge = gd / (py_o - py_i);
        float dx = ex[1] - ex[0];
        float tt = (px_i - ex[0]) / dx;
        float gtt = ge * (ey[1] - ey[0]);
        gsy[0] = ge * (1.f - tt); gsy[1] = ge * tt;
        gsx[0] = gtt * (tt - 1.f) / dx;
        gsx[1] = -gtt * tt / dx;
    }
    // screen -> clip: sx = (x/w * .5 + .5) W
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
        float q = qv[kk];
        float gX = gsx[kk] * 0.5f * W, gY = gsy[kk] * 0.5f * H;
        float* dp = dpb + 4 * (size_t)vv[kk];
        atomicAdd(dp + 0, gX * q);
        atomicAdd(dp + 1, gY * q);
        atomicAdd(dp + 3, -(gX * pc[kk].x + gY * pc[kk].y) * q * q);
    }
}

// Backward: the position gradient of the two pairs this pixel owns (right, down), added to d_pos (NULL: not wanted).  gb: the frame's g_out.
template <class Pre>
__device__ __forceinline__ void aa_owner_pairs_grad(const AAPixel& px, const Pre& pre, const float* gb, int C, const int* tri, float* d_pos, int pos_bstride,
                                                    int H, int W) {
    if (!d_pos) return;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        if (!px.pr[k].ok) continue;
        const int dirx = (k == 0) ? 1 : 0;
        // analysed again rather than read back from pr[k].h: hipcc 7.2 (-O2 / -O3) mis-compiles the edge data when it travels through the
        // struct array across the colour loop of the caller (wrong position gradients on the GPU, correct on the host build) -- the same
        // defect round 1 hit with a struct returned from the analysis loop
        const AAHit h = aa_analyse(px.rast_b, px.posb, tri, px.flags_b, px.x, px.y, dirx, H, W);
        if (!h.ok) continue;
        const float alpha = h.d - 0.5f;
        // wgt = |d - 0.5|: d wgt / d d = sign(d - 0.5), and 0 AT d == 0.5 (torch's abs').  That case is not exotic -- d is a difference
        // of pixel coordinates of magnitude 10^2..10^3, i.e. quantised to ~6e-5, so a few silhouette pairs per 10 renders sit exactly on
        // the midpoint -- and it matters: the outer pixel then keeps an exactly-zero value, F.normalize / cosine_similarity of a zero
        // normal hand back 1/eps-sized gradients (1e13) for it, and taking the +1 branch here sent them into the vertex positions
        // (|d total / d sdf weights| ~ 1e15 once every few dozen iterations; the oracle chain on the same batch stays O(1)).
        if (alpha == 0.f) continue;
        const int dst = (alpha >= 0.f) ? h.po : h.pi;
        const int src = (alpha >= 0.f) ? h.pi : h.po;
        const typename Pre::At at_src = pre.at(src), at_dst = pre.at(dst);
        float gw = 0.f;
        pre.channels([&](int ch, auto val) {
            const float g = gb[(size_t)dst * C + ch];
            if (g != 0.f) gw = fmaf(g, val(at_src) - val(at_dst), gw);
        });
        if (gw == 0.f) continue;
        aa_pos_grad(h, dirx, (alpha > 0.f) ? gw : -gw, px.posb, d_pos + (size_t)px.b * pos_bstride, H, W);
    }
}

// Phase 1 of the two plain kernels: this workgroup's pixel range [p0, p0 + AA_WG_PIX) of a [n][C] image copied with 16-byte accesses, or
// float by float where the range's float count or first float is no multiple of 4.
__device__ __forceinline__ void aa_copy_pixels(float* __restrict__ dst, const float* __restrict__ src, size_t p0, size_t n, int C) {
    const size_t cnt = (n - p0 < (size_t)AA_WG_PIX ? n - p0 : (size_t)AA_WG_PIX) * (size_t)C;   // floats of this workgroup's pixel range
    src += p0 * C;
    dst += p0 * C;
    if ((cnt & 3) == 0 && ((p0 * C) & 3) == 0) {
        for (size_t i = threadIdx.x; i < cnt / 4; i += 256) ((float4*)dst)[i] = ((const float4*)src)[i];
    } else {
        for (size_t i = threadIdx.x; i < cnt; i += 256) dst[i] = src[i];
    }
}

// the stored image of the two plain kernels; cb: its frame, C floats per pixel
struct AAStored {
    using At = int;
    const float* cb;
    int C;
    __device__ __forceinline__ At at(int p) const { return p; }
    template <class Fn>
    __device__ __forceinline__ void channels(Fn fn) const {
        for (int c = 0; c < C; ++c) fn(c, [&](At p) { return cb[(size_t)p * C + c]; });
    }
};

// Gather formulation: out[p] = color[p] + sum over the (at most four) pairs whose blended pixel is p of w (color[other] - color[p]).
// One pass, no atomics, deterministic: every workgroup copies its 256 pixels x C floats with 16-byte accesses (phase 1: the whole
// image except the ~1 % of pixels on an id discontinuity IS a copy), then the threads of pixels next to a discontinuity analyse their
// pairs and rewrite their own pixel (phase 2).  The scatter version this replaces (hipMemcpyAsync of the image + one thread per pair
// + fp32 atomics) moved the image twice more: 93 + 126 us per render at 4 x 1024^2 x 9 channels.
__global__ __launch_bounds__(256) void aa_fwd_kernel(const float* __restrict__ color, const float* __restrict__ rast, const float* __restrict__ pos,
                                                     int pos_bstride, const int* __restrict__ tri, const unsigned char* __restrict__ flags, int nf,
                                                     int nb, int H, int W, int C, float* __restrict__ out) {
    const size_t n = (size_t)nb * H * W;
    const size_t p0 = (size_t)blockIdx.x * AA_WG_PIX;
    aa_copy_pixels(out, color, p0, n, C);
    __syncthreads();                       // phase 2 overwrites pixels phase 1 (other threads of this workgroup) has just written
    for (int st = 0; st < AA_TILES; ++st) {
        AAPixel px;
        if (!aa_pixel<true>(px, p0 + (size_t)st * 256 + threadIdx.x, n, rast, pos, pos_bstride, tri, flags, nf, H, W)) continue;
        aa_blend(px, AAStored{color + px.gb0 * C, C}, out + (px.gb0 + px.self) * C);
    }
}

// Backward, same structure: g_color[p] = g[p] (1 - sum of the weights of the pairs that blend INTO p) + sum over the pairs that blend
// p's colour into their other pixel q of w g[q]  -- gathered, no atomics; the position gradient of a pair is added by the pair's owner.
__global__ __launch_bounds__(256) void aa_bwd_kernel(const float* __restrict__ color, const float* __restrict__ rast, const float* __restrict__ pos,
                                                     int pos_bstride, const int* __restrict__ tri, const unsigned char* __restrict__ flags, int nf,
                                                     int nb, int H, int W, int C, const float* __restrict__ g_out,
                                                     float* __restrict__ g_color, float* __restrict__ d_pos) {
    const size_t n = (size_t)nb * H * W;
    const size_t p0 = (size_t)blockIdx.x * AA_WG_PIX;
    aa_copy_pixels(g_color, g_out, p0, n, C);
    __syncthreads();
    for (int st = 0; st < AA_TILES; ++st) {
        AAPixel px;
        if (!aa_pixel<false>(px, p0 + (size_t)st * 256 + threadIdx.x, n, rast, pos, pos_bstride, tri, flags, nf, H, W)) continue;
        const float* gb = g_out + px.gb0 * C;
        if (aa_touched(px)) {
            float* grow = g_color + (px.gb0 + px.self) * C;
            for (int c = 0; c < C; ++c) grow[c] = aa_gather(px, gb, C, c);
        }
        aa_owner_pairs_grad(px, AAStored{color + px.gb0 * C, C}, gb, C, tri, d_pos, pos_bstride, H, W);
    }
}

// the composite of the layer buffers, evaluated at the pixel (composite.h: comp_value)
struct AAComposite {
    struct At { size_t i; bool cov; };        // global pixel index, coverage
    const CompArgs& a;
    const float* rast_b;
    size_t gb0, hw;
    __device__ __forceinline__ At at(int p) const { return {gb0 + p, rast_b[4 * (size_t)p + 3] > 0.f}; }
    template <class Fn>
    __device__ __forceinline__ void channels(Fn fn) const {
        int off = 0;
        for (int s_ = 0; s_ < a.n; ++s_) {
            const CompSrc& c = a.s[s_];
            const int wch = c.kind == 3 ? 1 : c.nch + 1;
            for (int j = 0; j < wch; ++j) fn(off + j, [&](const At& p) { return comp_value(c, j, p.i, p.cov, hw); });
            off += wch;
        }
    }
};

// Composite + antialias in ONE forward pass (no gradient: the buffers of a render nobody differentiates -- the nine dead buffers of a
// tick in its 'all' mode, the watertight validation render; render/render.py:375-382,430-449 run per buffer by the reference).  Phase 1
// composites the workgroup's pixels from the layer buffers straight into `out` (the separate composite pass wrote the stacked image and
// the antialias pass read it back and copied it: 2 x 151 MB per 4 x 1024^2 x 9-channel render, 4.4 x that with all 12 buffers); phase 2
// rewrites the ~1 % of pixels on a triangle-id discontinuity, evaluating the composite of the pair's other pixel on the fly.  Same
// arithmetic, in the same order, as composite_fwd_kernel followed by aa_fwd_kernel: bit-identical output.
__global__ __launch_bounds__(256) void aa_composite_fwd_kernel(CompArgs a, const float* __restrict__ rast, const float* __restrict__ pos,
                                                               int pos_bstride, const int* __restrict__ tri, const unsigned char* __restrict__ flags,
                                                               int nf, int nb, int H, int W, float* __restrict__ out) {
    D3H_DYN_SHARED(float, comp_lds);          // 256 * C floats
    const size_t hw = (size_t)H * W;
    const size_t n = (size_t)nb * hw;
    const size_t p0 = (size_t)blockIdx.x * AA_WG_PIX;
    const int C = a.C;
    for (int st = 0; st < AA_TILES; ++st) {
        const size_t first = p0 + (size_t)st * 256;
        if (first >= n) break;                                   // (workgroup-uniform)
        const size_t i = first + threadIdx.x;
        if (i < n) comp_row(a, rast, i, hw, comp_lds + (size_t)threadIdx.x * C);
        block_store_rows(out, comp_lds, first, n, C);
    }
    __syncthreads();                       // phase 2 overwrites pixels phase 1 (other threads of this workgroup) has just written
    for (int st = 0; st < AA_TILES; ++st) {
        AAPixel px;
        if (!aa_pixel<true>(px, p0 + (size_t)st * 256 + threadIdx.x, n, rast, pos, pos_bstride, tri, flags, nf, H, W)) continue;
        aa_blend(px, AAComposite{a, px.rast_b, px.gb0, hw}, out + (px.gb0 + px.self) * C);
    }
}

// The backward of the fused pass (a render somebody differentiates): antialias backward AND composite backward in one kernel.  The two
// separate kernels wrote the gradient of the stacked image (aa_bwd_kernel: g_color, nb x H x W x C floats) and read it straight back
// (composite_bwd_kernel) to slice it per source under the coverage mask -- 2 x 134 MB per backward at 4 x 1024^2 x 8 channels -- and the
// position gradient read the composited image the separate forward had stored; here the pre-antialias colours of the ~1 % pair pixels are
// re-evaluated from the layer buffers (comp_value), so the composited image is never materialised at all.  Same arithmetic in the same
// order as aa_bwd_kernel followed by composite_bwd_kernel: d(source) bit-identical, d_pos identical up to the order of its float atomics.
//   phase 1  d(src_k)[p][j] = covered(p) ? g_out[p][off_k + j] : 0     (rows staged through LDS both ways: 16-byte accesses)
//   phase 2  pixels on an id discontinuity recompute their own stacked gradient (gathered, as aa_bwd_kernel) and rewrite their entries;
//            the owner of a pair adds the pair's position gradient.
__global__ __launch_bounds__(256) void aa_composite_bwd_kernel(CompArgs a, const float* __restrict__ rast, const float* __restrict__ pos,
                                                               int pos_bstride, const int* __restrict__ tri, const unsigned char* __restrict__ flags,
                                                               int nf, int nb, int H, int W, const float* __restrict__ g_out, float* __restrict__ d_pos) {
    D3H_DYN_SHARED(float, cb_lds);            // 256 * C floats (the rows of g_out) + 256 * max(dch) floats (one source's block on its way out)
    const size_t hw = (size_t)H * W;
    const size_t n = (size_t)nb * hw;
    const size_t p0 = (size_t)blockIdx.x * AA_WG_PIX;
    const int C = a.C;
    float* rows = cb_lds;
    float* outb = cb_lds + 256 * C;
    for (int st = 0; st < AA_TILES; ++st) {
        const size_t first = p0 + (size_t)st * 256;
        if (first >= n) break;                                   // (workgroup-uniform)
        const size_t i = first + threadIdx.x;
        const bool cov = i < n ? rast[4 * i + 3] > 0.f : false;
        block_load_rows(rows, g_out, first, n, C);
        const float* gi = rows + (size_t)threadIdx.x * C;
        for (int k = 0; k < a.n; ++k) {
            const CompSrc& c = a.s[k];
            if (c.d) {                                           // (workgroup-uniform: kernel argument)
                if (i < n) {
                    for (int j = 0; j < c.nch; ++j) outb[threadIdx.x * c.dch + j] = cov ? gi[j] : 0.f;
                    for (int j = c.nch; j < c.dch; ++j) outb[threadIdx.x * c.dch + j] = 0.f;
                }
                block_store_rows(c.d, outb, first, n, c.dch);
            }
            gi += c.kind == 3 ? 1 : c.nch + 1;
        }
    }
    __syncthreads();                       // phase 2 overwrites entries phase 1 (other threads of this workgroup) has just written
    for (int st = 0; st < AA_TILES; ++st) {
        AAPixel px;
        if (!aa_pixel<false>(px, p0 + (size_t)st * 256 + threadIdx.x, n, rast, pos, pos_bstride, tri, flags, nf, H, W)) continue;
        const float* gb = g_out + px.gb0 * C;
        // ---- gradient of this pixel's stacked colour, sliced per source under its coverage ----
        if (aa_touched(px)) {
            const bool cov_s = px.rast_b[4 * (size_t)px.self + 3] > 0.f;
            int off = 0;
            for (int s_ = 0; s_ < a.n; ++s_) {
                const CompSrc& c = a.s[s_];
                if (c.d) {
                    for (int j = 0; j < c.nch; ++j) {
                        const float v = aa_gather(px, gb, C, off + j);
                        c.d[(px.gb0 + px.self) * c.dch + j] = cov_s ? v : 0.f;
                    }
                }
                off += c.kind == 3 ? 1 : c.nch + 1;
            }
        }
        aa_owner_pairs_grad(px, AAComposite{a, px.rast_b, px.gb0, hw}, gb, C, tri, d_pos, pos_bstride, H, W);
    }
}

// ---- one step of layered compositing (depth peeling, render/render.py:375-382 with more than one layer) ---------------------------------
// Layers are blended back to front; one step lays layer l over the image `under` [npix][C] of what lies behind it and antialiases the
// result along layer l's silhouettes:
//     pre[p]  = lerp(under[p], [src_k[p], 1], w[p])  per buffer k,   w[p] = covered_l(p) * alpha[p]   (alpha NULL: 1)
//     out     = antialias(pre, rast_l, pos, tri)
// kind 3 (the alpha-only 'msdf_image', one channel): pre = lerp(under, 1, covered * src); `alpha` does not enter.  The other kinds differ only in
// the background the host wrote into the deepest `under`; here they are one case.  The lerp is torch.lerp's two-branch form, exact at w = 0
// (under) and w = 1 (the source), so a layer that covers nothing is the identity.  Same shape as the fused pair above: pre[p] is a function
// of pixel p alone, so phase 2 re-evaluates the pair's other pixel and no pre-antialias image is stored.
__device__ __forceinline__ float layer_lerp(float a, float b, float w) { return w < 0.5f ? a + w * (b - a) : b - (b - a) * (1.0f - w); }

// pre-antialias value of channel j of source c at global pixel i; u = under + i * C + (first channel of the source), w = covered * alpha
__device__ __forceinline__ float layer_value(const CompSrc& c, int j, size_t i, bool cov, float w, const float* __restrict__ u) {
    if (!cov) return u[j];
    if (c.kind == 3) return layer_lerp(u[0], 1.0f, c.p[i * c.stride]);
    return layer_lerp(u[j], j < c.nch ? c.p[i * c.stride + j] : 1.0f, w);
}

// the layer blended over `under`, evaluated at the pixel
struct AALayer {
    struct At { size_t i; bool cov; float w; };       // global pixel index, coverage, alpha where covered
    const CompArgs& a;
    const float* alpha;
    const float* under;
    const float* rast_b;
    size_t gb0;
    __device__ __forceinline__ At at(int p) const {
        const bool cov = rast_b[4 * (size_t)p + 3] > 0.f;
        return {gb0 + p, cov, (cov && alpha) ? alpha[gb0 + p] : 1.0f};
    }
    template <class Fn>
    __device__ __forceinline__ void channels(Fn fn) const {
        int off = 0;
        for (int s_ = 0; s_ < a.n; ++s_) {
            const CompSrc& c = a.s[s_];
            const int wch = c.kind == 3 ? 1 : c.nch + 1;
            for (int j = 0; j < wch; ++j) fn(off + j, [&](const At& p) { return layer_value(c, j, p.i, p.cov, p.w, under + p.i * a.C + off); });
            off += wch;
        }
    }
};

__global__ __launch_bounds__(256) void layer_composite_fwd_kernel(CompArgs a, const float* __restrict__ alpha, const float* __restrict__ under,
                                                                  const float* __restrict__ rast, const float* __restrict__ pos, int pos_bstride,
                                                                  const int* __restrict__ tri, const unsigned char* __restrict__ flags, int nf, int nb,
                                                                  int H, int W, float* __restrict__ out) {
    D3H_DYN_SHARED(float, lay_lds);           // 256 * C floats: the rows of `under`, blended in place
    const size_t hw = (size_t)H * W;
    const size_t n = (size_t)nb * hw;
    const size_t p0 = (size_t)blockIdx.x * AA_WG_PIX;
    const int C = a.C;
    for (int st = 0; st < AA_TILES; ++st) {
        const size_t first = p0 + (size_t)st * 256;
        if (first >= n) break;                                   // (workgroup-uniform)
        const size_t i = first + threadIdx.x;
        block_load_rows(lay_lds, under, first, n, C);
        if (i < n && rast[4 * i + 3] > 0.f) {
            const float w = alpha ? alpha[i] : 1.0f;
            float* o = lay_lds + (size_t)threadIdx.x * C;
            for (int k = 0; k < a.n; ++k) {
                const CompSrc& c = a.s[k];
                const int wch = c.kind == 3 ? 1 : c.nch + 1;
                for (int j = 0; j < wch; ++j) o[j] = layer_value(c, j, i, true, w, o);
                o += wch;
            }
        }
        block_store_rows(out, lay_lds, first, n, C);
    }
    __syncthreads();                       // phase 2 overwrites pixels phase 1 (other threads of this workgroup) has just written
    for (int st = 0; st < AA_TILES; ++st) {
        AAPixel px;
        if (!aa_pixel<true>(px, p0 + (size_t)st * 256 + threadIdx.x, n, rast, pos, pos_bstride, tri, flags, nf, H, W)) continue;
        aa_blend(px, AALayer{a, alpha, under, px.rast_b, px.gb0}, out + (px.gb0 + px.self) * C);
    }
}

// Backward of the step.  Phase 1: every pixel as if no pair touched it (g = g_out[p]); the rows of g_out are staged in LDS and turned into
// the rows of d(under) in place, each source's block leaves through `outb` as in aa_composite_bwd_kernel, d(alpha) is one coalesced float per
// pixel.  `under` is read per lane (C consecutive floats of the lane's pixel) and only where alpha or a kind-3 source takes a gradient.  Phase 2:
// the pixels on an id discontinuity gather their pre-antialias gradient (as aa_bwd_kernel) and rewrite their own entries; the owner of a pair
// adds the pair's position gradient.  No atomics but those of d_pos.  dsrc[k], d_alpha, d_under may each be NULL: not written.
__global__ __launch_bounds__(256) void layer_composite_bwd_kernel(CompArgs a, const float* __restrict__ alpha, const float* __restrict__ under,
                                                                  const float* __restrict__ rast, const float* __restrict__ pos, int pos_bstride,
                                                                  const int* __restrict__ tri, const unsigned char* __restrict__ flags, int nf, int nb,
                                                                  int H, int W, const float* __restrict__ g_out, float* __restrict__ d_alpha,
                                                                  float* __restrict__ d_under, float* __restrict__ d_pos) {
    D3H_DYN_SHARED(float, lb_lds);            // 256 * C floats (rows of g_out -> rows of d_under) + 256 * max(dch) floats (one source's block on its way out)
    const size_t hw = (size_t)H * W;
    const size_t n = (size_t)nb * hw;
    const size_t p0 = (size_t)blockIdx.x * AA_WG_PIX;
    const int C = a.C;
    float* rows = lb_lds;
    float* outb = lb_lds + 256 * C;
    for (int st = 0; st < AA_TILES; ++st) {
        const size_t first = p0 + (size_t)st * 256;
        if (first >= n) break;                                   // (workgroup-uniform)
        const size_t i = first + threadIdx.x;
        const bool cov = i < n ? rast[4 * i + 3] > 0.f : false;
        const float w = cov ? (alpha ? alpha[i] : 1.0f) : 0.f;
        block_load_rows(rows, g_out, first, n, C);
        float* gi = rows + (size_t)threadIdx.x * C;
        const float* u = under + (i < n ? i : 0) * C;
        int off = 0;
        float da = 0.f;
        for (int k = 0; k < a.n; ++k) {
            const CompSrc& c = a.s[k];
            const int wch = c.kind == 3 ? 1 : c.nch + 1;
            if (i < n) {
                float* ob = outb + threadIdx.x * c.dch;
                if (c.kind == 3) {
                    if (c.d) ob[0] = cov ? gi[off] * (1.0f - u[off]) : 0.f;
                    if (d_under) gi[off] = gi[off] * (1.0f - (cov ? c.p[i * c.stride] : 0.f));
                } else {
                    for (int j = 0; j <= c.nch; ++j) {
                        const float gv = gi[off + j];
                        if (j < c.nch && c.d) ob[j] = gv * w;
                        if (d_alpha && cov) da += gv * ((j < c.nch ? c.p[i * c.stride + j] : 1.0f) - u[off + j]);
                        if (d_under) gi[off + j] = gv * (1.0f - w);
                    }
                }
                if (c.d) for (int j = c.kind == 3 ? 1 : c.nch; j < c.dch; ++j) ob[j] = 0.f;
            }
            if (c.d) block_store_rows(c.d, outb, first, n, c.dch);     // (workgroup-uniform)
            off += wch;
        }
        if (d_alpha && i < n) d_alpha[i] = da;
        if (d_under) block_store_rows(d_under, rows, first, n, C);
    }
    __syncthreads();                       // phase 2 overwrites entries phase 1 (other threads of this workgroup) has just written
    for (int st = 0; st < AA_TILES; ++st) {
        AAPixel px;
        if (!aa_pixel<false>(px, p0 + (size_t)st * 256 + threadIdx.x, n, rast, pos, pos_bstride, tri, flags, nf, H, W)) continue;
        const float* gb = g_out + px.gb0 * C;
        // ---- this pixel's gradients again, from the gathered gradient of its pre-antialias row ----
        if (aa_touched(px)) {
            const size_t is = px.gb0 + px.self;
            const bool cov_s = px.rast_b[4 * (size_t)px.self + 3] > 0.f;
            const float w_s = cov_s ? (alpha ? alpha[is] : 1.0f) : 0.f;
            const float* u = under + is * C;
            int off = 0;
            float da = 0.f;
            for (int s_ = 0; s_ < a.n; ++s_) {
                const CompSrc& c = a.s[s_];
                const int wch = c.kind == 3 ? 1 : c.nch + 1;
                for (int j = 0; j < wch; ++j) {
                    const float v = aa_gather(px, gb, C, off + j);
                    if (c.kind == 3) {
                        if (c.d) c.d[is * c.dch] = cov_s ? v * (1.0f - u[off]) : 0.f;
                        if (d_under) d_under[is * C + off] = v * (1.0f - (cov_s ? c.p[is * c.stride] : 0.f));
                    } else {
                        if (j < c.nch && c.d) c.d[is * c.dch + j] = v * w_s;
                        if (d_alpha && cov_s) da += v * ((j < c.nch ? c.p[is * c.stride + j] : 1.0f) - u[off + j]);
                        if (d_under) d_under[is * C + off + j] = v * (1.0f - w_s);
                    }
                }
                off += wch;
            }
            if (d_alpha) d_alpha[is] = da;
        }
        aa_owner_pairs_grad(px, AALayer{a, alpha, under, px.rast_b, px.gb0}, gb, C, tri, d_pos, pos_bstride, H, W);
    }
}

// ------------------------------------------------------------------------------------------------
// texture (2-D, bilinear, clamp)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void tex_fwd_kernel(const float* __restrict__ tex, int tex_bstride, int TH, int TW, int C,
                                                      const float* __restrict__ uv, size_t npix_total, size_t npix_per_b, float* __restrict__ out) {
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= npix_total) return;
    int b = (int)(i / npix_per_b);
    float u = uv[2 * i], v = uv[2 * i + 1];
    float x = u * TW - 0.5f, y = v * TH - 0.5f;
    float xf = floorf(x), yf = floorf(y);
    float fx = x - xf, fy = y - yf;
    int x0 = min(max((int)xf, 0), TW - 1), x1 = min(max((int)xf + 1, 0), TW - 1);
    int y0 = min(max((int)yf, 0), TH - 1), y1 = min(max((int)yf + 1, 0), TH - 1);
    const float* tb = tex + (size_t)b * tex_bstride;
    for (int c = 0; c < C; ++c) {
        float t00 = tb[((size_t)y0 * TW + x0) * C + c], t01 = tb[((size_t)y0 * TW + x1) * C + c];
        float t10 = tb[((size_t)y1 * TW + x0) * C + c], t11 = tb[((size_t)y1 * TW + x1) * C + c];
        out[i * C + c] = (t00 * (1.f - fx) + t01 * fx) * (1.f - fy) + (t10 * (1.f - fx) + t11 * fx) * fy;
    }
}

__global__ __launch_bounds__(256) void tex_bwd_kernel(int tex_bstride, int TH, int TW, int C, const float* __restrict__ uv, size_t npix_total,
                                                      size_t npix_per_b, const float* __restrict__ g_out, float* __restrict__ d_tex) {
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= npix_total) return;
    int b = (int)(i / npix_per_b);
    float u = uv[2 * i], v = uv[2 * i + 1];
    float x = u * TW - 0.5f, y = v * TH - 0.5f;
    float xf = floorf(x), yf = floorf(y);
    float fx = x - xf, fy = y - yf;
    int x0 = min(max((int)xf, 0), TW - 1), x1 = min(max((int)xf + 1, 0), TW - 1);
    int y0 = min(max((int)yf, 0), TH - 1), y1 = min(max((int)yf + 1, 0), TH - 1);
    float* tb = d_tex + (size_t)b * tex_bstride;
    for (int c = 0; c < C; ++c) {
        float g = g_out[i * C + c];
        if (g == 0.f) continue;
        atomicAdd(&tb[((size_t)y0 * TW + x0) * C + c], g * (1.f - fx) * (1.f - fy));
        atomicAdd(&tb[((size_t)y0 * TW + x1) * C + c], g * fx * (1.f - fy));
        atomicAdd(&tb[((size_t)y1 * TW + x0) * C + c], g * (1.f - fx) * fy);
        atomicAdd(&tb[((size_t)y1 * TW + x1) * C + c], g * fx * fy);
    }
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------
// pos: [nb or 1][nv][4] (pos_bstride = nv*4 or 0), tri [nf][3]; zbuf: nb*H*W uint64 scratch.
// big / big_cap: NULL / 0 = the wave-per-triangle rasteriser.  An int scratch of big_cap entries ASKS for the tile-binned rasteriser (large
// meshes; see raster_tile_kernel): it needs 3 NT + 8 ints of header (NT = nb * ceil(W / 32) * ceil(H / 32)) and one int per (triangle, tile)
// pair; when the pairs of this render do not fit the rest of the scratch the device falls back to the wave-per-triangle path by itself (no
// host read-back either way).  Both paths write bit-identical `rast` / `db`.
extern "C" int d3h_rasterize_fwd(const float* pos, int nv, int pos_bstride, const int* tri, int nf, int nb, int H, int W,
                                 unsigned long long* zbuf, int* big, int big_cap, float* rast, float* db, void* stream) {
    if (nb <= 0 || H <= 0 || W <= 0 || !rast || !zbuf) return D3H_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    size_t npix = (size_t)nb * H * W;
    const int kt_ = d3h_ktime_begin(D3H_KT_RASTER_FWD, (long long)(npix), (hipStream_t)(stream));
    const int tx_n = d3h_cdiv(W, BIN_T), ty_n = d3h_cdiv(H, BIN_T);
    const long long NT = (long long)nb * tx_n * ty_n;
    const int* flag = nullptr;
    if (big && nf > 0 && (long long)big_cap > 3 * NT + 8 + nf) {
        int *cnt = big, *off = cnt + NT, *cur = off + NT + 1, *fl = cur + NT, *pairs = fl + 4;
        const int cap = (int)((long long)big_cap - (3 * NT + 5));
        (void)hipMemsetAsync(cnt, 0, (size_t)NT * sizeof(int), s);
        hipLaunchKernelGGL((raster_bin_kernel<false>), dim3(d3h_cdiv(nf, 256), nb), dim3(256), 0, s, pos, pos_bstride, tri, nf, H, W, tx_n, ty_n, cnt,
                           (const int*)off, cur, (const int*)fl, pairs);
        hipLaunchKernelGGL(raster_bin_scan_kernel, dim3(1), dim3(1024), 0, s, (const int*)cnt, (int)NT, off, cur, fl, cap);
        hipLaunchKernelGGL((raster_bin_kernel<true>), dim3(d3h_cdiv(nf, 256), nb), dim3(256), 0, s, pos, pos_bstride, tri, nf, H, W, tx_n, ty_n, cnt,
                           (const int*)off, cur, (const int*)fl, pairs);
        hipLaunchKernelGGL(raster_tile_kernel, dim3(tx_n * ty_n, nb), dim3(256), 0, s, pos, pos_bstride, tri, H, W, tx_n, ty_n, (const int*)off,
                           (const int*)fl, pairs, rast, db);
        flag = fl;
    }
    (void)hipMemsetAsync(zbuf, 0xFF, npix * 8, s);
    if (nf > 0)
        hipLaunchKernelGGL(raster_tris_kernel, dim3(d3h_cdiv(nf, 4 * TRIS_PER_WAVE), nb), dim3(256), 0, s, pos, nv, pos_bstride, tri, nf, H, W, zbuf, flag);
    hipLaunchKernelGGL(raster_resolve_kernel, dim3(d3h_cdiv(npix, 256)), dim3(256), 0, s, pos, pos_bstride, tri, H, W, nb, zbuf, rast, db, flag);
    d3h_ktime_end(kt_, (hipStream_t)(stream));
    D3H_LAUNCH_CHECK();
    return D3H_OK;
}

// Depth peeling, first half: prev_key [nb][H][W] uint64 (overwritten; caller-owned scratch) = the (depth | id) key that the winner recorded in
// prev_rast [nb][H][W][4] -- a layer d3h_rasterize_fwd or d3h_rasterize_peel_fwd rendered from these pos / tri -- has at each pixel; ~0 where
// that layer is empty.  The same arithmetic as the rasteriser's, so the keys are bit-identical to the ones that won.
extern "C" int d3h_rasterize_peel_keys(const float* pos, int pos_bstride, const int* tri, int nf, int nb, int H, int W, const float* prev_rast,
                                       unsigned long long* prev_key, void* stream) {
    if (nb < 0 || H < 0 || W < 0 || nf < 0 || !prev_rast || !prev_key) return D3H_ERR_ARG;
    size_t npix = (size_t)nb * H * W;
    if (npix == 0) return D3H_OK;
    hipLaunchKernelGGL(raster_peel_key_kernel, dim3(d3h_cdiv(npix, 256)), dim3(256), 0, (hipStream_t)stream, pos, pos_bstride, tri, nf, H, W, nb,
                       prev_rast, prev_key);
    D3H_LAUNCH_CHECK();
    return D3H_OK;
}

// One layer of depth peeling and / or range mode, on the wave-per-triangle rasteriser; writes rast / db as d3h_rasterize_fwd (db may be NULL).
//  - prev_rast (or NULL): the previous layer.  Its keys go to prev_key [nb][H][W] uint64 (caller-owned scratch; d3h_rasterize_peel_keys) and
//    each pixel then reports the covering fragment with the smallest key strictly greater than its previous key.  prev_rast NULL and
//    prev_key non-NULL: prev_key already holds those keys.  Both NULL: no peeling (the first layer).
//  - ranges [nb][2] int32 (device; or NULL) = (start, count) into tri per frame: range mode.  pos is [nv][4], shared (pos_bstride must be 0),
//    max_count >= every count (it sizes the grid), and every range lies inside [0, nf] -- a range outside it rasterises nothing.  The ids in
//    rast are absolute (tri index + 1).  ranges NULL: the frames rasterise all nf triangles, max_count is ignored.
//  zbuf: nb*H*W uint64 scratch.  The backward of every layer is d3h_rasterize_bwd / d3h_rasterize_bwd_db with the same pos_bstride.
extern "C" int d3h_rasterize_peel_fwd(const float* pos, int pos_bstride, const int* tri, int nf, int nb, int H, int W, const int* ranges,
                                      int max_count, const float* prev_rast, unsigned long long* prev_key, unsigned long long* zbuf, float* rast,
                                      float* db, void* stream) {
    if (nb <= 0 || H <= 0 || W <= 0 || nf < 0 || !rast || !zbuf) return D3H_ERR_ARG;
    if (ranges && (pos_bstride != 0 || max_count < 0 || max_count > nf)) return D3H_ERR_ARG;
    if (prev_rast && !prev_key) return D3H_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    size_t npix = (size_t)nb * H * W;
    if (prev_rast)
        hipLaunchKernelGGL(raster_peel_key_kernel, dim3(d3h_cdiv(npix, 256)), dim3(256), 0, s, pos, pos_bstride, tri, nf, H, W, nb, prev_rast, prev_key);
    (void)hipMemsetAsync(zbuf, 0xFF, npix * 8, s);
    const int ntri = ranges ? max_count : nf;
    if (ntri > 0)
        hipLaunchKernelGGL(raster_tris_peel_kernel, dim3(d3h_cdiv(ntri, 4 * TRIS_PER_WAVE), nb), dim3(256), 0, s, pos, pos_bstride, tri, nf, ranges, H, W,
                           (const unsigned long long*)prev_key, zbuf);
    hipLaunchKernelGGL(raster_resolve_kernel, dim3(d3h_cdiv(npix, 256)), dim3(256), 0, s, pos, pos_bstride, tri, H, W, nb, (const unsigned long long*)zbuf,
                       rast, db, (const int*)nullptr);
    D3H_LAUNCH_CHECK();
    return D3H_OK;
}

// d_pos accumulated (caller zero-fills)
extern "C" int d3h_rasterize_bwd(const float* pos, int pos_bstride, const int* tri, int nb, int H, int W, const float* rast,
                                 const float* g_rast, float* d_pos, void* stream) {
    size_t npix = (size_t)nb * H * W;
    const int kt_ = d3h_ktime_begin(D3H_KT_RASTER_BWD, (long long)(npix), (hipStream_t)(stream));
    hipLaunchKernelGGL(raster_bwd_kernel, dim3(d3h_cdiv(npix, 256)), dim3(256), 0, (hipStream_t)stream, pos, pos_bstride, tri, H, W, nb, rast,
                       g_rast, d_pos);
    d3h_ktime_end(kt_, (hipStream_t)(stream));
    D3H_LAUNCH_CHECK();
    return D3H_OK;
}

// d3h_rasterize_bwd with the gradient of the pixel derivatives: g_rast [nb][H][W][4] (d(u, v); may be NULL) and g_db [nb][H][W][4]
// (d(du/dX, du/dY, dv/dX, dv/dY); may be NULL) -> d_pos, accumulated (caller zero-fills)
extern "C" int d3h_rasterize_bwd_db(const float* pos, int pos_bstride, const int* tri, int nb, int H, int W, const float* rast,
                                    const float* g_rast, const float* g_db, float* d_pos, void* stream) {
    if (nb < 0 || H < 0 || W < 0 || !d_pos) return D3H_ERR_ARG;
    size_t npix = (size_t)nb * H * W;
    if (npix == 0 || (!g_rast && !g_db)) return D3H_OK;
    hipLaunchKernelGGL(raster_bwd_db_kernel, dim3(d3h_cdiv(npix, 256)), dim3(256), 0, (hipStream_t)stream, pos, pos_bstride, tri, H, W, nb, rast,
                       g_rast, g_db, d_pos);
    D3H_LAUNCH_CHECK();
    return D3H_OK;
}

// attr [nb or 1][nv][na] (attr_bstride = nv*na or 0); out [nb][H][W][na]; out_da [nb][H][W][2 na] (optional, needs db)
extern "C" int d3h_interpolate_fwd(const float* attr, int attr_bstride, int na, const float* rast, const int* tri, const float* db, int nb,
                                   int H, int W, float* out, float* out_da, void* stream) {
    size_t npb = (size_t)H * W, n = npb * nb;
    if (n == 0) return D3H_OK;
    hipLaunchKernelGGL((interp_fwd_kernel<0>), dim3(d3h_cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, attr, attr_bstride, na, rast, tri, db,
                       n, npb, out, out_da);
    D3H_LAUNCH_CHECK();
    return D3H_OK;
}

// d_attr accumulated (caller zero-fills; may be NULL); d_rast [nb][H][W][4] overwritten (may be NULL)
extern "C" int d3h_interpolate_bwd(const float* attr, int attr_bstride, int na, const float* rast, const int* tri, const float* g_out, int nb,
                                   int H, int W, float* d_attr, float* d_rast, void* stream) {
    size_t npb = (size_t)H * W, n = npb * nb;
    if (n == 0) return D3H_OK;
    hipLaunchKernelGGL(interp_bwd_kernel, dim3(d3h_cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, attr, attr_bstride, na, rast, tri, g_out, n,
                       npb, d_attr, d_rast);
    D3H_LAUNCH_CHECK();
    return D3H_OK;
}

// d3h_interpolate_fwd with the pixel derivatives of a list of channels: idx [nidx] int32, each in [0, na) (NULL: every channel in order,
// nidx = na); out [nb][H][W][na] and out_da [nb][H][W][2 nidx] overwritten, pair k = (d attr[idx[k]] / dX, d attr[idx[k]] / dY) from
// db [nb][H][W][4]
extern "C" int d3h_interpolate_fwd_da(const float* attr, int attr_bstride, int na, const float* rast, const int* tri, const float* db,
                                      const int* idx, int nidx, int nb, int H, int W, float* out, float* out_da, void* stream) {
    if (nb < 0 || H < 0 || W < 0 || na < 0 || nidx < 0 || (!idx && nidx != na)) return D3H_ERR_ARG;
    size_t npb = (size_t)H * W, n = npb * nb;
    if (n == 0) return D3H_OK;
    if (!rast || !out || !out_da || !db) return D3H_ERR_ARG;
    hipLaunchKernelGGL(interp_fwd_da_kernel, dim3(d3h_cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, attr, attr_bstride, na, rast, tri, db,
                       idx, nidx, n, npb, out, out_da);
    D3H_LAUNCH_CHECK();
    return D3H_OK;
}

// d3h_interpolate_bwd with the gradient of the attribute pixel derivatives: g_out [nb][H][W][na] (may be NULL), g_da [nb][H][W][2 nidx]
// (may be NULL; needs db) for the channels idx [nidx] of d3h_interpolate_fwd_da (NULL: every channel, nidx = na).  d_attr accumulated
// (caller zero-fills; may be NULL); d_rast [nb][H][W][4] and d_db [nb][H][W][4] overwritten, zero where nothing is covered (may be NULL)
extern "C" int d3h_interpolate_bwd_da(const float* attr, int attr_bstride, int na, const float* rast, const int* tri, const float* db,
                                      const int* idx, int nidx, const float* g_out, const float* g_da, int nb, int H, int W, float* d_attr,
                                      float* d_rast, float* d_db, void* stream) {
    if (nb < 0 || H < 0 || W < 0 || na < 0 || nidx < 0 || (!idx && nidx != na) || (g_da && !db)) return D3H_ERR_ARG;
    size_t npb = (size_t)H * W, n = npb * nb;
    if (n == 0) return D3H_OK;
    if (!rast) return D3H_ERR_ARG;
    hipLaunchKernelGGL(interp_bwd_da_kernel, dim3(d3h_cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, attr, attr_bstride, na, rast, tri, db,
                       idx, nidx, g_out, g_da, n, npb, d_attr, d_rast, d_db);
    D3H_LAUNCH_CHECK();
    return D3H_OK;
}

// All interpolations of one render layer in one pass (render/render.py:257-267,283,328 + the coverage mask of :66).  attr [nb or 1][nv][na]
// packs the vertex attributes; group g = the next width_g channels, written to out_g [nb][H][W][width_g] (NULL: not produced; unused
// trailing groups have width 0).  face_attr [nb or 1][nf][fw] is gathered by triangle id into face_out [nb][H][W][fw] (both may be
// NULL); mask_out [nb][H][W] = rast[..., 3] > 0 (may be NULL).
extern "C" int d3h_gbuffer_fwd(const float* attr, int attr_bstride, int na, const float* face_attr, int face_bstride, int fw, const float* rast,
                               const int* tri, int nb, int H, int W, float* out0, int w0, float* out1, int w1, float* out2, int w2, float* out3,
                               int w3, float* face_out, float* mask_out, void* stream) {
    if (w0 < 0 || w1 < 0 || w2 < 0 || w3 < 0 || w0 + w1 + w2 + w3 != na || (face_out && (!face_attr || fw <= 0))) return D3H_ERR_ARG;
    size_t npb = (size_t)H * W, n = npb * nb;
    if (n == 0) return D3H_OK;
    GbufOut o{{out0, out1, out2, out3}, {w0, w1, w2, w3}, face_out, mask_out};
    const int kt_ = d3h_ktime_begin(D3H_KT_GBUFFER_FWD, (long long)n, (hipStream_t)stream);
    hipLaunchKernelGGL(gbuffer_fwd_kernel, dim3(d3h_cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, attr, attr_bstride, na, face_attr,
                       face_bstride, fw, rast, tri, n, npb, o);
    d3h_ktime_end(kt_, (hipStream_t)stream);
    D3H_LAUNCH_CHECK();
    return D3H_OK;
}

// The LDS-summing backward (gbuffer_bwd_tile_kernel), unless switched off.  Read per call, for A/B runs and tests in one process:
//   D3H_GBUF_LDS=0        the per-row kernel (returns false: the caller launches it)
//   D3H_GBUF_TILE=WxH     tile shape: 16x16 (default), 32x8, 64x4, 8x32, 32x32 (4 pixels per thread)
//   D3H_GBUF_LDS_SLOTS=n  at most n slots per table (rounded down to a power of two; 0: every contribution takes the direct-atomic path);
//                         default GBL_SLOTS -- the tuning table is in profiles/image_bwd_tail_ab.txt
static inline int gbl_pow2_floor(int v) { int p = 0; for (int q = 1; q > 0 && q <= v; q <<= 1) p = q; return p; }
template <bool RAST>
static bool gbuffer_bwd_tile_launch(const float* attr, int attr_bstride, int na, int face_bstride, int fw, const float* rast, const int* tri, int nb,
                                    int H, int W, const GbufGrad& gg, float* d_attr, float* d_face, float* d_rast, const float* pos, int pos_bstride,
                                    float* d_pos, hipStream_t s) {
    const char* e = getenv("D3H_GBUF_LDS");
    if ((e && e[0] == '0') || nb > 65535) return false;
    e = getenv("D3H_GBUF_LDS_SLOTS");
    const int limit = e ? atoi(e) : GBL_SLOTS;
    const int vstride = (d_attr ? na : 0) + (RAST ? 3 : 0);
    const int vcap = (vstride > 0 && limit > 0) ? gbl_pow2_floor(std::min(std::min(limit, GBL_VCAP), GBL_VPOOL / vstride)) : 0;
    const int fcap = (fw > 0 && limit > 0) ? gbl_pow2_floor(std::min(std::min(limit, GBL_FCAP), GBL_FPOOL / fw)) : 0;
    e = getenv("D3H_GBUF_TILE");
    const int tw = e ? atoi(e) : 16, th = (e && strchr(e, 'x')) ? atoi(strchr(e, 'x') + 1) : 16;
#define GBL_LAUNCH(TW, TH)                                                                                                                         \
    hipLaunchKernelGGL((gbuffer_bwd_tile_kernel<RAST, TW, TH>), dim3(d3h_cdiv(W, TW), d3h_cdiv(H, TH), nb), dim3(256), 0, s, attr, attr_bstride, na, \
                       face_bstride, fw, rast, tri, gg, d_attr, d_face, d_rast, pos, pos_bstride, H, W, d_pos, vcap, fcap)
    if (tw == 64 && th == 4) GBL_LAUNCH(64, 4);
    else if (tw == 8 && th == 32) GBL_LAUNCH(8, 32);
    else if (tw == 32 && th == 32) GBL_LAUNCH(32, 32);
    else if (tw == 32 && th == 8) GBL_LAUNCH(32, 8);
    else GBL_LAUNCH(16, 16);
#undef GBL_LAUNCH
    return true;
}

// g_k: upstream gradient of group k (NULL = zero); d_attr, d_face accumulated (caller zero-fills; may be NULL); d_rast [nb][H][W][4]
// overwritten (may be NULL)
extern "C" int d3h_gbuffer_bwd(const float* attr, int attr_bstride, int na, int face_bstride, int fw, const float* rast, const int* tri, int nb,
                               int H, int W, const float* g0, int w0, const float* g1, int w1, const float* g2, int w2, const float* g3, int w3,
                               const float* g_face, float* d_attr, float* d_face, float* d_rast, void* stream) {
    if (w0 < 0 || w1 < 0 || w2 < 0 || w3 < 0 || w0 + w1 + w2 + w3 != na) return D3H_ERR_ARG;
    size_t npb = (size_t)H * W, n = npb * nb;
    if (n == 0) return D3H_OK;
    GbufGrad gg{{g0, g1, g2, g3}, {w0, w1, w2, w3}, g_face};
    const int kt = d3h_ktime_begin(D3H_KT_GBUFFER_BWD, (long long)n, (hipStream_t)stream);
    if (!gbuffer_bwd_tile_launch<false>(attr, attr_bstride, na, face_bstride, fw, rast, tri, nb, H, W, gg, d_attr, d_face, d_rast, nullptr, 0, nullptr,
                                        (hipStream_t)stream))
        hipLaunchKernelGGL((gbuffer_bwd_kernel<false>), dim3(d3h_cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, attr, attr_bstride, na, face_bstride,
                           fw, rast, tri, n, npb, gg, d_attr, d_face, d_rast, (const float*)nullptr, 0, H, W, (float*)nullptr);
    d3h_ktime_end(kt, (hipStream_t)stream);
    D3H_LAUNCH_CHECK();
    return D3H_OK;
}

// d3h_gbuffer_bwd AND d3h_rasterize_bwd of the raster the G-buffer was interpolated from, in one pass: the barycentric gradient of every
// covered pixel goes into d_pos (same layout as pos; accumulated -- the caller zero-fills) instead of a [nb][H][W][4] image.  For a render
// whose raster has no other differentiable consumer (render/render.py:257-267 -- every interpolation of the layer is in this one pass).
extern "C" int d3h_gbuffer_raster_bwd(const float* attr, int attr_bstride, int na, int face_bstride, int fw, const float* rast, const int* tri, int nb,
                                      int H, int W, const float* g0, int w0, const float* g1, int w1, const float* g2, int w2, const float* g3, int w3,
                                      const float* g_face, float* d_attr, float* d_face, const float* pos, int pos_bstride, float* d_pos,
                                      void* stream) {
    if (w0 < 0 || w1 < 0 || w2 < 0 || w3 < 0 || w0 + w1 + w2 + w3 != na || !pos || !d_pos) return D3H_ERR_ARG;
    size_t npb = (size_t)H * W, n = npb * nb;
    if (n == 0) return D3H_OK;
    GbufGrad gg{{g0, g1, g2, g3}, {w0, w1, w2, w3}, g_face};
    const int kt = d3h_ktime_begin(D3H_KT_GBUFFER_BWD, (long long)n, (hipStream_t)stream);
    if (!gbuffer_bwd_tile_launch<true>(attr, attr_bstride, na, face_bstride, fw, rast, tri, nb, H, W, gg, d_attr, d_face, nullptr, pos, pos_bstride, d_pos,
                                       (hipStream_t)stream))
        hipLaunchKernelGGL((gbuffer_bwd_kernel<true>), dim3(d3h_cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, attr, attr_bstride, na, face_bstride,
                           fw, rast, tri, n, npb, gg, d_attr, d_face, (float*)nullptr, pos, pos_bstride, H, W, d_pos);
    d3h_ktime_end(kt, (hipStream_t)stream);
    D3H_LAUNCH_CHECK();
    return D3H_OK;
}

// hash table: keys [cap] uint64, vals [2 cap] int32, cap = power of two >= 4 * 3 nf
extern "C" int d3h_antialias_hash(const int* tri, int nf, unsigned long long* keys, int* vals, int cap, void* stream) {
    if (cap <= 0 || (cap & (cap - 1))) return D3H_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    const int kt_ = d3h_ktime_begin(D3H_KT_AA_PREP, (long long)(nf), (hipStream_t)(stream));
    if ((const char*)vals == (const char*)keys + (size_t)cap * 8) {           // one allocation (d3h/raster.py:_hash_for): one fill
        (void)hipMemsetAsync(keys, 0xFF, (size_t)cap * 16, s);
    } else {
        (void)hipMemsetAsync(keys, 0xFF, (size_t)cap * 8, s);
        (void)hipMemsetAsync(vals, 0xFF, (size_t)cap * 8, s);
    }
    if (nf > 0) hipLaunchKernelGGL(aa_hash_build_kernel, dim3(d3h_cdiv(3 * (int64_t)nf, 256)), dim3(256), 0, s, tri, nf, keys, vals, (unsigned)(cap - 1));
    d3h_ktime_end(kt_, (hipStream_t)(stream));
    D3H_LAUNCH_CHECK();
    return D3H_OK;
}

// flags [nb][nf] uint8 (overwritten): the per-frame silhouette-edge bits of every triangle (bit e: edge (e, e+1)), from the edge hash of
// d3h_antialias_hash and the clip-space positions pos [nb or 1][nv][4] (pos_bstride floats between frames, 0 = shared)
extern "C" int d3h_antialias_flags(const float* pos, int pos_bstride, const int* tri, int nf, int nb, const unsigned long long* keys,
                                   const int* vals, int cap, int H, int W, unsigned char* flags, void* stream) {
    if (cap <= 0 || (cap & (cap - 1))) return D3H_ERR_ARG;
    if (nf <= 0 || nb <= 0) return D3H_OK;
    hipLaunchKernelGGL(aa_edge_flags_kernel, dim3(d3h_cdiv((int64_t)nf * nb, 256)), dim3(256), 0, (hipStream_t)stream, pos, pos_bstride, tri, nf, nb,
                       keys, vals, (unsigned)(cap - 1), H, W, flags);
    D3H_LAUNCH_CHECK();
    return D3H_OK;
}

extern "C" int d3h_antialias_fwd(const float* color, const float* rast, const float* pos, int pos_bstride, const int* tri, int nf,
                                 const unsigned char* flags, int nb, int H, int W, int C, float* out, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    size_t n = (size_t)nb * H * W;
    if (n == 0) return D3H_OK;
    const int kt = d3h_ktime_begin(D3H_KT_AA_FWD, (long long)n * C, s);
    hipLaunchKernelGGL(aa_fwd_kernel, dim3(d3h_cdiv(n, AA_WG_PIX)), dim3(256), 0, s, color, rast, pos, pos_bstride, tri, flags, nf, nb, H, W, C, out);
    d3h_ktime_end(kt, s);
    D3H_LAUNCH_CHECK();
    return D3H_OK;
}

// the frame and mesh arguments of the four fused entry points: refused?  (nf == 0 is allowed without pos / tri / flags: an empty mesh has no
// triangles, nothing is covered, nothing to blend)
static inline bool aa_frame_args_bad(int nb, int H, int W, int nf, const float* pos, const int* tri, const unsigned char* flags) {
    return nb < 0 || H <= 0 || W <= 0 || nf < 0 || (nf > 0 && (!pos || !tri || !flags));
}

// Composite (d3h_composite_fwd: same source description, host arrays read before the call returns) AND antialias (d3h_antialias_fwd:
// flags from d3h_antialias_flags) in one forward pass; out [nb][H][W][C], C = sum(nch + 1) (kind 3: 1).  No backward: for renders nobody
// differentiates.  Bit-identical to the two separate calls.
extern "C" int d3h_composite_antialias_fwd(int nsrc, const float* const* src, const int* stride, const int* nch, const int* kind,
                                           const float* const* bg, const int* bg_batched, const float* rast, const float* pos, int pos_bstride,
                                           const int* tri, int nf, const unsigned char* flags, int nb, int H, int W, float* out, void* stream) {
    CompArgs a;
    int rc = comp_args(a, nsrc, src, nullptr, stride, nch, kind, bg, bg_batched, true);
    if (rc != D3H_OK || !src || !rast || !out || aa_frame_args_bad(nb, H, W, nf, pos, tri, flags)) return D3H_ERR_ARG;
    for (int k = 0; k < nsrc; ++k) if (!src[k]) return D3H_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    size_t n = (size_t)nb * H * W;
    if (n == 0) return D3H_OK;
    const int kt = d3h_ktime_begin(D3H_KT_AA_FWD, (long long)n * a.C, s);
    hipLaunchKernelGGL(aa_composite_fwd_kernel, dim3(d3h_cdiv(n, AA_WG_PIX)), dim3(256), (size_t)256 * a.C * sizeof(float), s, a, rast, pos, pos_bstride,
                       tri, flags, nf, nb, H, W, out);
    d3h_ktime_end(kt, s);
    D3H_LAUNCH_CHECK();
    return D3H_OK;
}

// Backward of d3h_composite_antialias_fwd for a render somebody differentiates (same source description; dsrc[k]: dense [nb][H][W][dch[k]]
// gradient buffer of source k or NULL, fully overwritten; dch NULL = nch, dch[k] > nch[k]: the source is the channel prefix of a wider tensor
// whose gradient this is -- the trailing channels are zero-filled; d_pos accumulated -- the caller zero-fills -- or NULL): antialias backward
// and composite backward in one pass; d(source) bit-identical to d3h_antialias_bwd followed by d3h_composite_bwd.
extern "C" int d3h_composite_antialias_bwd(int nsrc, const float* const* src, float* const* dsrc, const int* dch, const int* stride, const int* nch, const int* kind,
                                           const float* const* bg, const int* bg_batched, const float* rast, const float* pos, int pos_bstride,
                                           const int* tri, int nf, const unsigned char* flags, int nb, int H, int W, const float* g_out, float* d_pos,
                                           void* stream) {
    CompArgs a;
    int rc = comp_args(a, nsrc, src, dsrc, stride, nch, kind, bg, bg_batched, true, dch);
    if (rc != D3H_OK || !src || !dsrc || !rast || !g_out || aa_frame_args_bad(nb, H, W, nf, pos, tri, flags)) return D3H_ERR_ARG;
    int maxch = 1;
    for (int k = 0; k < nsrc; ++k) {
        if (!src[k]) return D3H_ERR_ARG;
        if (a.s[k].dch > maxch) maxch = a.s[k].dch;
    }
    hipStream_t s = (hipStream_t)stream;
    size_t n = (size_t)nb * H * W;
    if (n == 0) return D3H_OK;
    const int kt = d3h_ktime_begin(D3H_KT_AA_BWD, (long long)n * a.C, s);
    hipLaunchKernelGGL(aa_composite_bwd_kernel, dim3(d3h_cdiv(n, AA_WG_PIX)), dim3(256), (size_t)256 * (a.C + maxch) * sizeof(float), s, a, rast, pos,
                       pos_bstride, tri, flags, nf, nb, H, W, g_out, d_pos);
    d3h_ktime_end(kt, s);
    D3H_LAUNCH_CHECK();
    return D3H_OK;
}

// One step of layered compositing (depth peeling): out [nb][H][W][C] = antialias(lerp(under, [src_k, 1], covered * alpha) per source k, rast,
// pos, tri), C = sum(nch + 1) (kind 3: 1, lerp(under, 1, covered * src), alpha does not enter).  Sources as d3h_composite_antialias_fwd
// (host arrays; kind 0..3, where 0..2 are one case here: the background is what the caller wrote into `under` [nb][H][W][C]); alpha
// [nb][H][W] or NULL = 1; rast the layer's raster, flags from d3h_antialias_flags.  The lerp is exact at weight 0 and 1.  `out` must not
// alias `under`.  C is limited to 64 (the rows of a 256-pixel tile in 64 KB of LDS).
extern "C" int d3h_layer_composite_antialias_fwd(int nsrc, const float* const* src, const int* stride, const int* nch, const int* kind,
                                                 const float* alpha, const float* under, const float* rast, const float* pos, int pos_bstride,
                                                 const int* tri, int nf, const unsigned char* flags, int nb, int H, int W, float* out, void* stream) {
    CompArgs a;
    int rc = comp_args(a, nsrc, src, nullptr, stride, nch, kind, nullptr, nullptr, false);
    if (rc != D3H_OK || !src || !under || !rast || !out || out == under || aa_frame_args_bad(nb, H, W, nf, pos, tri, flags))
        return D3H_ERR_ARG;
    for (int k = 0; k < nsrc; ++k) if (!src[k]) return D3H_ERR_ARG;
    const size_t lds = (size_t)256 * a.C * sizeof(float);
    if (lds > 65536) return D3H_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    size_t n = (size_t)nb * H * W;
    if (n == 0) return D3H_OK;
    const int kt = d3h_ktime_begin(D3H_KT_AA_FWD, (long long)n * a.C, s);
    hipLaunchKernelGGL(layer_composite_fwd_kernel, dim3(d3h_cdiv(n, AA_WG_PIX)), dim3(256), lds, s, a, alpha, under, rast, pos, pos_bstride, tri, flags,
                       nf, nb, H, W, out);
    d3h_ktime_end(kt, s);
    D3H_LAUNCH_CHECK();
    return D3H_OK;
}

// Backward of d3h_layer_composite_antialias_fwd (same description; g_out [nb][H][W][C]).  dsrc[k] [nb][H][W][dch[k]] (dch NULL = nch; wider:
// trailing channels zero-filled), d_alpha [nb][H][W], d_under [nb][H][W][C]: each overwritten completely, or NULL = not wanted and not
// written (dsrc itself may be NULL); d_pos accumulated -- the caller zero-fills -- or NULL.  d(src) = g w, d(under) = g (1 - w), d(alpha) =
// covered * sum over the sources of kind 0..2 and their channels of g (end - under), g the gradient of the pre-antialias row; no atomics
// but those of d_pos.  C + max(dch) is limited to 64.
extern "C" int d3h_layer_composite_antialias_bwd(int nsrc, const float* const* src, float* const* dsrc, const int* dch, const int* stride, const int* nch,
                                                 const int* kind, const float* alpha, const float* under, const float* rast, const float* pos,
                                                 int pos_bstride, const int* tri, int nf, const unsigned char* flags, int nb, int H, int W,
                                                 const float* g_out, float* d_alpha, float* d_under, float* d_pos, void* stream) {
    CompArgs a;
    int rc = comp_args(a, nsrc, src, dsrc, stride, nch, kind, nullptr, nullptr, false, dch);
    if (rc != D3H_OK || !src || !under || !rast || !g_out || d_under == g_out || aa_frame_args_bad(nb, H, W, nf, pos, tri, flags))
        return D3H_ERR_ARG;
    int maxch = 1;
    for (int k = 0; k < nsrc; ++k) {
        if (!src[k]) return D3H_ERR_ARG;
        if (a.s[k].d && a.s[k].dch > maxch) maxch = a.s[k].dch;
    }
    const size_t lds = (size_t)256 * (a.C + maxch) * sizeof(float);
    if (lds > 65536) return D3H_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    size_t n = (size_t)nb * H * W;
    if (n == 0) return D3H_OK;
    const int kt = d3h_ktime_begin(D3H_KT_AA_BWD, (long long)n * a.C, s);
    hipLaunchKernelGGL(layer_composite_bwd_kernel, dim3(d3h_cdiv(n, AA_WG_PIX)), dim3(256), lds, s, a, alpha, under, rast, pos, pos_bstride, tri, flags,
                       nf, nb, H, W, g_out, d_alpha, d_under, d_pos);
    d3h_ktime_end(kt, s);
    D3H_LAUNCH_CHECK();
    return D3H_OK;
}

// g_color overwritten; d_pos accumulated (caller zero-fills; may be NULL)
extern "C" int d3h_antialias_bwd(const float* color, const float* rast, const float* pos, int pos_bstride, const int* tri, int nf,
                                 const unsigned char* flags, int nb, int H, int W, int C, const float* g_out, float* g_color, float* d_pos,
                                 void* stream) {
    hipStream_t s = (hipStream_t)stream;
    size_t n = (size_t)nb * H * W;
    if (n == 0) return D3H_OK;
    const int kt_ = d3h_ktime_begin(D3H_KT_AA_BWD, (long long)(n * C), s);
    hipLaunchKernelGGL(aa_bwd_kernel, dim3(d3h_cdiv(n, AA_WG_PIX)), dim3(256), 0, s, color, rast, pos, pos_bstride, tri, flags, nf, nb, H, W, C, g_out,
                       g_color, d_pos);
    d3h_ktime_end(kt_, s);
    D3H_LAUNCH_CHECK();
    return D3H_OK;
}

extern "C" int d3h_texture_fwd(const float* tex, int tex_bstride, int TH, int TW, int C, const float* uv, int nb, int H, int W, float* out,
                               void* stream) {
    size_t npb = (size_t)H * W, n = npb * nb;
    if (n == 0) return D3H_OK;
    hipLaunchKernelGGL(tex_fwd_kernel, dim3(d3h_cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, tex, tex_bstride, TH, TW, C, uv, n, npb, out);
    D3H_LAUNCH_CHECK();
    return D3H_OK;
}

// d_tex accumulated (caller zero-fills)
extern "C" int d3h_texture_bwd(int tex_bstride, int TH, int TW, int C, const float* uv, int nb, int H, int W, const float* g_out, float* d_tex,
                               void* stream) {
    size_t npb = (size_t)H * W, n = npb * nb;
    if (n == 0) return D3H_OK;
    hipLaunchKernelGGL(tex_bwd_kernel, dim3(d3h_cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, tex_bstride, TH, TW, C, uv, n, npb, g_out, d_tex);
    D3H_LAUNCH_CHECK();
    return D3H_OK;
}
