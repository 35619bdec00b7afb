// denoise.hip -- the cross-bilateral denoiser of render.optixutils, forward and backward.
//
// Replaces (reference file:line): render/optixutils/c_src/denoising.cu:14-72 (bilateral_denoiser_fwd_kernel), :74-130 (.._bwd_kernel).
// Tap radius r = 2 ceil(2.5 sigma) + 1; weight of tap t for the centre c:
//     exp(-|t - c|^2 / (2 sigma^2)) * clamp(n_t . n_c, 1e-4, 1)^128 * exp(-|z_t - z_c| / max(dz * |t - c|, 1e-4))
// with dz = zdz.y of the CENTRE in the forward.  out = {sum of w col_t, max(sum of w, 1e-4)}.  The backward is the exact adjoint as a gather:
// d col_c = sum over taps of w' g_t, where w' is the weight the forward gave c as a tap of t -- the same expression with dz of the TAP.
// Taps outside the image are skipped.
//
// At sigma = 2 a pixel reads 23 x 23 taps of 8 floats.  A workgroup owns a 16 x 16 tile and stages {col or g, nrm, zdz} of the tile plus its halo in
// LDS (one plane per channel), in bands of as many rows as fit DN_LDS_FLOATS, so global memory is read once per band rather than once per tap.
#include "d3h_vec.h"

namespace {

constexpr int DN_T = 16;                      // tile edge
constexpr int DN_LDS_FLOATS = 12288;          // 48 KB of staging
constexpr float DN_EPS = 0.0001f;

// v: forward col [B][H][W][3], backward g [B][H][W][4] (its first three channels); out: forward [B][H][W][4], backward d col [B][H][W][3]
template <bool BWD>
__global__ __launch_bounds__(256) void denoise_kernel(const float* __restrict__ v, const float* __restrict__ nrm, const float* __restrict__ zdz, int H, int W,
                                                      float sigma, int rad, int band, float* __restrict__ out) {
    __shared__ float tile[DN_LDS_FLOATS];
    const int tx = threadIdx.x & (DN_T - 1), ty = threadIdx.x >> 4;
    const int x0 = blockIdx.x * DN_T, y0 = blockIdx.y * DN_T, b = blockIdx.z;
    const int x = x0 + tx, y = y0 + ty;
    const bool live = x < W && y < H;
    const size_t img = (size_t)b * H * W;
    const int TW = DN_T + 2 * rad;                                 // staged columns: x0 - rad .. x0 + 15 + rad
    const int vch = BWD ? 4 : 3;
    const int PS = band * TW;                                      // the 8 staged channels are planes of PS floats: a wave's taps are consecutive words
    V3 cn = mk(0.f, 0.f, 0.f);
    float cz = 0.f, cdz = 0.f;
    if (live) {
        cn = ld3(nrm + 3 * (img + (size_t)y * W + x));
        cz = zdz[2 * (img + (size_t)y * W + x)];
        cdz = zdz[2 * (img + (size_t)y * W + x) + 1];
    }
    const float inv2var = 1.0f / (2.0f * sigma * sigma);
    V3 acc = mk(0.f, 0.f, 0.f);
    float accw = 0.f;
    // bands of staged rows: image rows r0 .. r0 + band - 1 of the window y0 - rad .. y0 + 15 + rad
    for (int r0 = y0 - rad; r0 <= y0 + DN_T - 1 + rad; r0 += band) {
        const int r1 = min(r0 + band, y0 + DN_T + rad);              // one past the band's last row
        __syncthreads();
        for (int k = threadIdx.x; k < (r1 - r0) * TW; k += 256) {
            const int sy = r0 + k / TW, sx = x0 - rad + k % TW;
            float* t = tile + k;
            if (sy >= 0 && sy < H && sx >= 0 && sx < W) {
                const size_t q = img + (size_t)sy * W + sx;
                t[0] = v[vch * q]; t[PS] = v[vch * q + 1]; t[2 * PS] = v[vch * q + 2];
                t[3 * PS] = nrm[3 * q]; t[4 * PS] = nrm[3 * q + 1]; t[5 * PS] = nrm[3 * q + 2];
                t[6 * PS] = zdz[2 * q]; t[7 * PS] = zdz[2 * q + 1];
            }
        }
        __syncthreads();
        if (!live) continue;
        const int fy0 = max(max(r0, y - rad), 0), fy1 = min(min(r1 - 1, y + rad), H - 1);
        const int fx0 = max(x - rad, 0), fx1 = min(x + rad, W - 1);
        for (int sy = fy0; sy <= fy1; ++sy) {
            const int row = (sy - r0) * TW - (x0 - rad);
            const float dy = (float)(sy - y);
            for (int sx = fx0; sx <= fx1; ++sx) {
                const float* t = tile + (row + sx);
                const float dx = (float)(sx - x);
                const float d2 = dx * dx + dy * dy, dist = sqrtf(d2);
                const float w_xy = expf(-d2 * inv2var);
                const float c = fminf(fmaxf(t[3 * PS] * cn.x + t[4 * PS] * cn.y + t[5 * PS] * cn.z, DN_EPS), 1.0f);
                float c2 = c * c, c4 = c2 * c2, c8 = c4 * c4, c16 = c8 * c8, c32 = c16 * c16, c64 = c32 * c32;
                const float w_n = c64 * c64;
                const float w_z = expf(-(fabsf(t[6 * PS] - cz) / fmaxf((BWD ? t[7 * PS] : cdz) * dist, DN_EPS)));
                const float w = w_xy * w_n * w_z;
                acc = acc + mk(t[0], t[PS], t[2 * PS]) * w;
                accw += w;
            }
        }
    }
    if (!live) return;
    const size_t q = img + (size_t)y * W + x;
    if (BWD) st3(out + 3 * q, acc);
    else { st3(out + 4 * q, acc); out[4 * q + 3] = fmaxf(accw, DN_EPS); }
}

// The same filter for TWO images under one set of guides (the demodulated path denoises diffuse and specular light with identical normals and
// depths): the guide planes are staged once and each tap's weight -- two exp and a 128th power -- is computed once for both.  11 staged planes
// instead of 8.  Same tap order (rows ascending, then columns, whatever the band height) and the same weight and accumulation expressions as
// denoise_kernel, so each image's result equals the single-image launch's bit for bit.  DN2_LDS_FLOATS: 52 KB, so that three workgroups still
// share a CU's 160 KB as they do with the single-image kernel's 48 KB; at sigma = 2 (a 38 x 38 window) that is 31 rows per band, two bands.
constexpr int DN2_LDS_FLOATS = 13312;

template <bool BWD>
__global__ __launch_bounds__(256) void denoise2_kernel(const float* __restrict__ va, const float* __restrict__ vb, const float* __restrict__ nrm,
                                                       const float* __restrict__ zdz, int H, int W, float sigma, int rad, int band, float* __restrict__ outa,
                                                       float* __restrict__ outb) {
    __shared__ float tile[DN2_LDS_FLOATS];
    const int tx = threadIdx.x & (DN_T - 1), ty = threadIdx.x >> 4;
    const int x0 = blockIdx.x * DN_T, y0 = blockIdx.y * DN_T, b = blockIdx.z;
    const int x = x0 + tx, y = y0 + ty;
    const bool live = x < W && y < H;
    const size_t img = (size_t)b * H * W;
    const int TW = DN_T + 2 * rad;
    const int vch = BWD ? 4 : 3;
    const int PS = band * TW;                                      // planes: 0-2 image a, 3-5 image b, 6-8 normal, 9-10 (z, dz)
    V3 cn = mk(0.f, 0.f, 0.f);
    float cz = 0.f, cdz = 0.f;
    if (live) {
        cn = ld3(nrm + 3 * (img + (size_t)y * W + x));
        cz = zdz[2 * (img + (size_t)y * W + x)];
        cdz = zdz[2 * (img + (size_t)y * W + x) + 1];
    }
    const float inv2var = 1.0f / (2.0f * sigma * sigma);
    V3 acc = mk(0.f, 0.f, 0.f), bcc = mk(0.f, 0.f, 0.f);
    float accw = 0.f;
    for (int r0 = y0 - rad; r0 <= y0 + DN_T - 1 + rad; r0 += band) {
        const int r1 = min(r0 + band, y0 + DN_T + rad);
        __syncthreads();
        for (int k = threadIdx.x; k < (r1 - r0) * TW; k += 256) {
            const int sy = r0 + k / TW, sx = x0 - rad + k % TW;
            float* t = tile + k;
            if (sy >= 0 && sy < H && sx >= 0 && sx < W) {
                const size_t q = img + (size_t)sy * W + sx;
                t[0] = va[vch * q]; t[PS] = va[vch * q + 1]; t[2 * PS] = va[vch * q + 2];
                t[3 * PS] = vb[vch * q]; t[4 * PS] = vb[vch * q + 1]; t[5 * PS] = vb[vch * q + 2];
                t[6 * PS] = nrm[3 * q]; t[7 * PS] = nrm[3 * q + 1]; t[8 * PS] = nrm[3 * q + 2];
                t[9 * PS] = zdz[2 * q]; t[10 * PS] = zdz[2 * q + 1];
            }
        }
        __syncthreads();
        if (!live) continue;
        const int fy0 = max(max(r0, y - rad), 0), fy1 = min(min(r1 - 1, y + rad), H - 1);
        const int fx0 = max(x - rad, 0), fx1 = min(x + rad, W - 1);
        for (int sy = fy0; sy <= fy1; ++sy) {
            const int row = (sy - r0) * TW - (x0 - rad);
            const float dy = (float)(sy - y);
            for (int sx = fx0; sx <= fx1; ++sx) {
                const float* t = tile + (row + sx);
                const float dx = (float)(sx - x);
                const float d2 = dx * dx + dy * dy, dist = sqrtf(d2);
                const float w_xy = expf(-d2 * inv2var);
                const float c = fminf(fmaxf(t[6 * PS] * cn.x + t[7 * PS] * cn.y + t[8 * PS] * cn.z, DN_EPS), 1.0f);
                float c2 = c * c, c4 = c2 * c2, c8 = c4 * c4, c16 = c8 * c8, c32 = c16 * c16, c64 = c32 * c32;
                const float w_n = c64 * c64;
                const float w_z = expf(-(fabsf(t[9 * PS] - cz) / fmaxf((BWD ? t[10 * PS] : cdz) * dist, DN_EPS)));
                const float w = w_xy * w_n * w_z;
                acc = acc + mk(t[0], t[PS], t[2 * PS]) * w;
                bcc = bcc + mk(t[3 * PS], t[4 * PS], t[5 * PS]) * w;
                accw += w;
            }
        }
    }
    if (!live) return;
    const size_t q = img + (size_t)y * W + x;
    if (BWD) { st3(outa + 3 * q, acc); st3(outb + 3 * q, bcc); }
    else {
        st3(outa + 4 * q, acc); outa[4 * q + 3] = fmaxf(accw, DN_EPS);
        st3(outb + 4 * q, bcc); outb[4 * q + 3] = fmaxf(accw, DN_EPS);
    }
}

// the tap radius 2 ceil(2.5 sigma) + 1, the product taken in double as the reference's host-promoted expression takes it
inline int denoise_radius(float sigma) { return 2 * (int)ceil((double)sigma * 2.5) + 1; }

}  // namespace

// Cross-bilateral filter of col [B][H][W][3] guided by nrm [B][H][W][3] and zdz [B][H][W][2] (depth, depth gradient).  backward = 0: out [B][H][W][4]
// := {weighted colour sum, max(weight sum, 1e-4)}.  backward = 1: `col` is the gradient g [B][H][W][4] of that output and out [B][H][W][3] := d col
// (the exact adjoint, a gather: no atomics; g's fourth channel does not reach col).  sigma > 0; a radius whose window row does not fit the staging
// buffer (sigma > ~150) is an argument error.
extern "C" int d3h_bilateral_denoise(const float* col, const float* nrm, const float* zdz, int B, int H, int W, float sigma, int backward, float* out,
                                     void* stream) {
    if (B < 0 || H < 0 || W < 0 || !(sigma > 0.0f) || backward < 0 || backward > 1) return D3H_ERR_ARG;
    if ((size_t)B * H * W == 0) return D3H_OK;
    if (!col || !nrm || !zdz || !out || B > 65535) return D3H_ERR_ARG;
    const int rad = denoise_radius(sigma);
    const int TW = DN_T + 2 * rad;
    const int band = DN_LDS_FLOATS / (8 * TW);
    if (rad < 1 || band < 1) return D3H_ERR_ARG;
    dim3 grid((unsigned)d3h_cdiv(W, DN_T), (unsigned)d3h_cdiv(H, DN_T), (unsigned)B);
    hipStream_t s = (hipStream_t)stream;
    if (backward) hipLaunchKernelGGL(denoise_kernel<true>, grid, dim3(256), 0, s, col, nrm, zdz, H, W, sigma, rad, band, out);
    else hipLaunchKernelGGL(denoise_kernel<false>, grid, dim3(256), 0, s, col, nrm, zdz, H, W, sigma, rad, band, out);
    D3H_LAUNCH_CHECK();
    return D3H_OK;
}

// d3h_bilateral_denoise for n = 1 or 2 images that share the guides nrm / zdz, one launch: cols[i] and outs[i] are HOST arrays of n device pointers,
// each image and output laid out as col / out there.  Image i's output equals d3h_bilateral_denoise(cols[i], ...)'s bit for bit; with n = 2 the
// guides are staged and every tap weight is computed once instead of twice.
extern "C" int d3h_bilateral_denoise_n(const float* const* cols, int n, const float* nrm, const float* zdz, int B, int H, int W, float sigma, int backward,
                                       float* const* outs, void* stream) {
    if (!cols || !outs || n < 1 || n > 2) return D3H_ERR_ARG;
    if (n == 1) return d3h_bilateral_denoise(cols[0], nrm, zdz, B, H, W, sigma, backward, outs[0], stream);
    if (B < 0 || H < 0 || W < 0 || !(sigma > 0.0f) || backward < 0 || backward > 1) return D3H_ERR_ARG;
    if ((size_t)B * H * W == 0) return D3H_OK;
    if (!cols[0] || !cols[1] || !nrm || !zdz || !outs[0] || !outs[1] || B > 65535) return D3H_ERR_ARG;
    const int rad = denoise_radius(sigma);
    const int TW = DN_T + 2 * rad;
    const int band = DN2_LDS_FLOATS / (11 * TW);
    if (rad < 1 || band < 1) return D3H_ERR_ARG;
    dim3 grid((unsigned)d3h_cdiv(W, DN_T), (unsigned)d3h_cdiv(H, DN_T), (unsigned)B);
    hipStream_t s = (hipStream_t)stream;
    if (backward) hipLaunchKernelGGL(denoise2_kernel<true>, grid, dim3(256), 0, s, cols[0], cols[1], nrm, zdz, H, W, sigma, rad, band, outs[0], outs[1]);
    else hipLaunchKernelGGL(denoise2_kernel<false>, grid, dim3(256), 0, s, cols[0], cols[1], nrm, zdz, H, W, sigma, rad, band, outs[0], outs[1]);
    D3H_LAUNCH_CHECK();
    return D3H_OK;
}
