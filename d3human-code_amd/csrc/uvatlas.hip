// uvatlas.hip -- textured-mesh export: a closed-form triangle-pair UV atlas, the position bake into it, and the 2 x 2 mip op of Texture2D.
//
// Replaces (reference file:line): the xatlas.parametrize call + render_uv + two util.dilate(.., 7) of train.py:198-246 (xatlas_uvmap), and
// render/texture.py:20-30 (texture2d_mip: avg_pool_nhwc forward, a bilinear x2 upsample of 0.25 dout as the backward).
//
// The atlas.  All layout arithmetic is in whole texels of the H x W texture.  Two triangles share one square cell of s x s texels
// (s >= 5, chosen by the host: the largest s with floor(W/s) floor(H/s) >= ceil(F/2); nx = W / s cells per row).  Triangle f lives in
// cell c = f / 2 at (cx, cy) = (c % nx, c / nx), in half h = f % 2.  The three slots of half 0 are q0 = (1,1), q1 = (s-3,1), q2 = (1,s-3)
// (texel-corner coordinates inside the cell); half 1 has (s,s) - qk, a half turn, so the orientation is kept.  Corner (r + k) % 3 of the
// face takes slot k, r the corner opposite the longest edge (the largest angle sits on the right angle: least shear).
//
// The bake.  A texel centre (x, y) of the cell belongs to half 0 iff x + y <= s.  Its barycentrics in ITS OWN triangle are
// b1 = (x - 1) / (s - 4), b2 = (y - 1) / (s - 4), b0 = 1 - b1 - b2 (after the half turn for half 1), NOT clamped: the gutter texels carry
// the affine extrapolation of their own triangle.  A point of a triangle's uv image is at least one texel (max-norm) from the border of
// its half cell, so the four taps of a level-0 bilinear lookup all read texels of that one affine map: the lookup reproduces it exactly,
// with no seam and no dilation.  (Price: (s-4)^2 / s^2 of the texels carry surface; mip levels above 0 mix triangles.)
// Everything up to the barycentrics is integer arithmetic in HALF texels (x2 = 2 x is an odd integer), so ownership, the half, `inside`
// and the numerators of b0, b1, b2 are exact; each barycentric is one rounded division.
//
// No LDS, no atomics, no scratch: one thread per triangle / texel / output element.
#include "d3h_common.h"

namespace {

constexpr int UA_T = 256;

__device__ __forceinline__ int64_t ua_index(const void* __restrict__ tri, int idx64, int64_t i) {
    return idx64 ? ((const int64_t*)tri)[i] : (int64_t)((const int*)tri)[i];
}

// squared length of a - b in float32, summed left to right
__device__ __forceinline__ float ua_len2(const float* a, const float* b) {
    const float dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
    return dx * dx + dy * dy + dz * dz;
}

// one thread per triangle: rot[f], the three uv pairs of its corners, and the identity texture-index row
__global__ __launch_bounds__(UA_T) void uvatlas_layout_kernel(const float* __restrict__ v_pos, int64_t V, const void* __restrict__ tri, int idx64, int64_t F,
                                                              int s, int nx, int H, int W, float* __restrict__ uvs, int64_t* __restrict__ t_tex_idx,
                                                              unsigned char* __restrict__ rot) {
    const int64_t f = (int64_t)blockIdx.x * UA_T + threadIdx.x;
    if (f >= F) return;
    const int64_t i0 = ua_index(tri, idx64, 3 * f), i1 = ua_index(tri, idx64, 3 * f + 1), i2 = ua_index(tri, idx64, 3 * f + 2);
    int r = 0;
    if (i0 >= 0 && i0 < V && i1 >= 0 && i1 < V && i2 >= 0 && i2 < V) {            // an index outside the vertex array is not followed: r = 0
        float p[3][3];
        for (int k = 0; k < 3; ++k) { p[0][k] = v_pos[3 * i0 + k]; p[1][k] = v_pos[3 * i1 + k]; p[2][k] = v_pos[3 * i2 + k]; }
        // edge opposite corner k; `>` is false on NaN and on ties, so the lowest corner index wins and a degenerate triangle gets 0
        const float l0 = ua_len2(p[1], p[2]), l1 = ua_len2(p[2], p[0]), l2 = ua_len2(p[0], p[1]);
        float best = l0;
        if (l1 > best) { r = 1; best = l1; }
        if (l2 > best) r = 2;
    }
    rot[f] = (unsigned char)r;
    const int64_t c = f >> 1;
    const int h = (int)(f & 1);
    const int cx = (int)(c % nx), cy = (int)(c / nx);
    const int qx[3] = {1, s - 3, 1}, qy[3] = {1, 1, s - 3};
    const float fw = (float)W, fh = (float)H;
    for (int k = 0; k < 3; ++k) {
        const int X = cx * s + (h ? s - qx[k] : qx[k]), Y = cy * s + (h ? s - qy[k] : qy[k]);
        int corner = r + k;
        if (corner >= 3) corner -= 3;
        uvs[2 * (3 * f + corner)] = (float)X / fw;
        uvs[2 * (3 * f + corner) + 1] = (float)Y / fh;
        t_tex_idx[3 * f + k] = 3 * f + k;
    }
}

// one thread per texel (i along W, j along H)
__global__ __launch_bounds__(UA_T) void uvatlas_bake_kernel(const float* __restrict__ v_pos, int64_t V, const void* __restrict__ tri, int idx64, int64_t F,
                                                            const unsigned char* __restrict__ rot, int s, int nx, int ny, int H, int W,
                                                            float* __restrict__ pos, float* __restrict__ owned, float* __restrict__ inside,
                                                            int* __restrict__ tri_out) {
    const int64_t t = (int64_t)blockIdx.x * UA_T + threadIdx.x;
    if (t >= (int64_t)H * W) return;
    const int i = (int)(t % W), j = (int)(t / W);
    const int cx = i / s, cy = j / s;
    float o = 0.f, in = 0.f, p0 = 0.f, p1 = 0.f, p2 = 0.f;
    int fo = -1;
    if (cx < nx && cy < ny) {
        int x2 = 2 * (i - cx * s) + 1, y2 = 2 * (j - cy * s) + 1;               // twice the texel centre inside the cell: odd, 1 .. 2 s - 1
        const int h = (x2 + y2 <= 2 * s) ? 0 : 1;
        const int64_t f = 2 * ((int64_t)cy * nx + cx) + h;
        if (f < F) {
            if (h) { x2 = 2 * s - x2; y2 = 2 * s - y2; }
            const int den = 2 * (s - 4), n1 = x2 - 2, n2 = y2 - 2, n0 = den - n1 - n2;
            const float b0 = (float)n0 / (float)den, b1 = (float)n1 / (float)den, b2 = (float)n2 / (float)den;
            o = 1.f;
            fo = (int)f;
            in = (n0 >= 0 && n1 >= 0 && n2 >= 0) ? 1.f : 0.f;
            int r = rot[f];
            if (r > 2) r = 0;
            int64_t v[3];
            bool ok = true;
            for (int k = 0; k < 3; ++k) {
                v[k] = ua_index(tri, idx64, 3 * f + (r + k) % 3);
                ok = ok && v[k] >= 0 && v[k] < V;
            }
            if (ok) {
                const float* a = v_pos + 3 * v[0];
                const float* b = v_pos + 3 * v[1];
                const float* c = v_pos + 3 * v[2];
                p0 = b0 * a[0] + b1 * b[0] + b2 * c[0];
                p1 = b0 * a[1] + b1 * b[1] + b2 * c[1];
                p2 = b0 * a[2] + b1 * b[2] + b2 * c[2];
            }
        }
    }
    pos[3 * t] = p0;
    pos[3 * t + 1] = p1;
    pos[3 * t + 2] = p2;
    owned[t] = o;
    inside[t] = in;
    tri_out[t] = fo;
}

// one thread per output element of the 2 x 2 mean, NHWC
__global__ __launch_bounds__(UA_T) void mip2x2_fwd_kernel(const float* __restrict__ x, int64_t total, int h, int w, int C, float* __restrict__ y) {
    const int64_t t = (int64_t)blockIdx.x * UA_T + threadIdx.x;
    if (t >= total) return;
    const int c = (int)(t % C);
    const int64_t u = t / C;
    const int ox = (int)(u % w);
    const int64_t q = u / w;
    const int oy = (int)(q % h);
    const int64_t n = q / h;
    const int64_t row = (int64_t)2 * w * C;                                        // one fine row
    const float* b = x + (n * 2 * h + 2 * oy) * row + (int64_t)2 * ox * C + c;
    y[t] = ((b[0] + b[C]) + (b[row] + b[row + C])) * 0.25f;
}

// one thread per element of the FINE gradient [N][2h][2w][C]: the bilinear x2 upsample of 0.25 dout at texel centres, indices clamped at the
// border (weights 0.75 / 0.25: the coarse texel the fine one lies in, and its neighbour on the fine texel's side)
__global__ __launch_bounds__(UA_T) void mip2x2_bwd_kernel(const float* __restrict__ dy, int64_t total, int h, int w, int C, float* __restrict__ dx) {
    const int64_t t = (int64_t)blockIdx.x * UA_T + threadIdx.x;
    if (t >= total) return;
    const int c = (int)(t % C);
    const int64_t u = t / C;
    const int fx = (int)(u % (2 * w));
    const int64_t q = u / (2 * w);
    const int fy = (int)(q % (2 * h));
    const int64_t n = q / (2 * h);
    const int x0 = fx >> 1, y0 = fy >> 1;
    const int x1 = min(max(x0 + ((fx & 1) ? 1 : -1), 0), w - 1), y1 = min(max(y0 + ((fy & 1) ? 1 : -1), 0), h - 1);
    const float* b = dy + n * h * (int64_t)w * C + c;
    const float a00 = b[((int64_t)y0 * w + x0) * C], a01 = b[((int64_t)y0 * w + x1) * C];
    const float a10 = b[((int64_t)y1 * w + x0) * C], a11 = b[((int64_t)y1 * w + x1) * C];
    dx[t] = (0.75f * (0.75f * a00 + 0.25f * a01) + 0.25f * (0.75f * a10 + 0.25f * a11)) * 0.25f;
}

inline bool ua_misaligned(const void* p, size_t a) { return ((uintptr_t)p & (a - 1)) != 0; }

}  // namespace

// Triangle-pair atlas of F triangles tri [F][3] (int32, or int64 with idx64 != 0) over v_pos [V][3] in an H x W texture with cells of s >= 5 texels,
// nx = W / s cells per row (the caller chose s so that nx (H / s) >= ceil(F / 2); checked).  Overwritten: uvs [3 F][2] (corner j of face f at row
// 3 f + j; each coordinate one correctly rounded division of two integers), t_tex_idx [F][3] int64 (= 3 f + j), rot [F] uint8 (the corner
// opposite the longest edge, squared lengths in float32, ties and NaN to the lowest index; a face with an index outside [0, V) gets 0).
// One launch, one thread per triangle.  F == 0 is a no-op.
extern "C" int d3h_uvatlas_layout(const float* v_pos, int64_t V, const void* tri, int idx64, int64_t F, int s, int nx, int H, int W, float* uvs,
                                  int64_t* t_tex_idx, unsigned char* rot, void* stream) {
    if (F < 0 || V < 0 || H < 1 || W < 1 || s < 5 || nx < 1 || (int64_t)nx * s > W) return D3H_ERR_ARG;
    if (F == 0) return D3H_OK;
    if (!v_pos || !tri || !uvs || !t_tex_idx || !rot) return D3H_ERR_ARG;
    if (ua_misaligned(v_pos, 4) || ua_misaligned(tri, idx64 ? 8 : 4) || ua_misaligned(uvs, 4) || ua_misaligned(t_tex_idx, 8)) return D3H_ERR_ARG;
    const int64_t cells = (F + 1) / 2, ny = H / s;
    if (cells > (int64_t)nx * ny || (F + UA_T - 1) / UA_T > 0x7fffffff) return D3H_ERR_ARG;
    hipLaunchKernelGGL(uvatlas_layout_kernel, dim3((unsigned)((F + UA_T - 1) / UA_T)), dim3(UA_T), 0, (hipStream_t)stream, v_pos, V, tri, idx64, F, s, nx, H, W,
                       uvs, t_tex_idx, rot);
    D3H_LAUNCH_CHECK();
    return D3H_OK;
}

// Position bake into the atlas of d3h_uvatlas_layout (same s, nx, ny = cell rows, H, W; rot [F] from it; v_pos may be another pose of the same
// faces).  Overwritten, per texel: pos [H][W][3] (the affine map of the owning triangle, extrapolated in its gutter; 0 where unowned or where the
// face has an index outside [0, V)), owned [H][W] and inside [H][W] as 0 / 1 floats, tri_out [H][W] int32 (the owning face, -1 = none).
// One launch, one thread per texel.
extern "C" int d3h_uvatlas_bake(const float* v_pos, int64_t V, const void* tri, int idx64, int64_t F, const unsigned char* rot, int s, int nx, int ny,
                                int H, int W, float* pos, float* owned, float* inside, int* tri_out, void* stream) {
    if (F < 0 || V < 0 || H < 1 || W < 1 || s < 5 || nx < 0 || ny < 0 || (int64_t)nx * s > W || (int64_t)ny * s > H || F > 0x7fffffff) return D3H_ERR_ARG;
    if (!pos || !owned || !inside || !tri_out || (F > 0 && (!v_pos || !tri || !rot))) return D3H_ERR_ARG;
    if (ua_misaligned(v_pos, 4) || ua_misaligned(tri, idx64 ? 8 : 4) || ua_misaligned(pos, 4) || ua_misaligned(owned, 4) || ua_misaligned(inside, 4) ||
        ua_misaligned(tri_out, 4))
        return D3H_ERR_ARG;
    const int64_t n = (int64_t)H * W;
    if ((n + UA_T - 1) / UA_T > 0x7fffffff) return D3H_ERR_ARG;
    hipLaunchKernelGGL(uvatlas_bake_kernel, dim3((unsigned)((n + UA_T - 1) / UA_T)), dim3(UA_T), 0, (hipStream_t)stream, v_pos, V, tri, idx64, F, rot, s, nx, ny,
                       H, W, pos, owned, inside, tri_out);
    D3H_LAUNCH_CHECK();
    return D3H_OK;
}

// y [N][h][w][C] := the 2 x 2 mean of x [N][2 h][2 w][C] (overwritten).  One thread per output element.
extern "C" int d3h_mip2x2_fwd(const float* x, int64_t N, int h, int w, int C, float* y, void* stream) {
    if (N < 0 || h < 1 || w < 1 || C < 1 || h > 0x3fffffff || w > 0x3fffffff) return D3H_ERR_ARG;
    if (N == 0) return D3H_OK;
    if (!x || !y || ua_misaligned(x, 4) || ua_misaligned(y, 4)) return D3H_ERR_ARG;
    if (N > INT64_MAX / 4 / h / w / C) return D3H_ERR_ARG;
    const int64_t total = N * h * w * C;
    if ((total + UA_T - 1) / UA_T > 0x7fffffff) return D3H_ERR_ARG;
    hipLaunchKernelGGL(mip2x2_fwd_kernel, dim3((unsigned)((total + UA_T - 1) / UA_T)), dim3(UA_T), 0, (hipStream_t)stream, x, total, h, w, C, y);
    D3H_LAUNCH_CHECK();
    return D3H_OK;
}

// dx [N][2 h][2 w][C] := the bilinear x2 upsample (texel centres, border clamped) of 0.25 dy [N][h][w][C] (overwritten): the gradient rule of the
// reference's texture2d_mip, which is NOT the adjoint of the forward.  One thread per element of dx.
extern "C" int d3h_mip2x2_bwd(const float* dy, int64_t N, int h, int w, int C, float* dx, void* stream) {
    if (N < 0 || h < 1 || w < 1 || C < 1 || h > 0x3fffffff || w > 0x3fffffff) return D3H_ERR_ARG;
    if (N == 0) return D3H_OK;
    if (!dy || !dx || ua_misaligned(dy, 4) || ua_misaligned(dx, 4)) return D3H_ERR_ARG;
    if (N > INT64_MAX / 16 / h / w / C) return D3H_ERR_ARG;
    const int64_t total = N * 4 * h * w * C;
    if ((total + UA_T - 1) / UA_T > 0x7fffffff) return D3H_ERR_ARG;
    hipLaunchKernelGGL(mip2x2_bwd_kernel, dim3((unsigned)((total + UA_T - 1) / UA_T)), dim3(UA_T), 0, (hipStream_t)stream, dy, total, h, w, C, dx);
    D3H_LAUNCH_CHECK();
    return D3H_OK;
}
