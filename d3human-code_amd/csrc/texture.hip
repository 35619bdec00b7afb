// texture.hip -- the full nvdiffrast texture op: mip pyramids, nearest / bilinear / trilinear lookups, wrap / clamp / zero / cube boundaries,
// gradients for the texture levels, uv, uv_da and the mip level bias.  The contract is stated in d3h/texture.py; the bilinear / clamp
// lookup without mips and without a uv gradient stays in raster.hip (d3h_texture_fwd / _bwd) and is not routed here.
//
// Storage: the levels of a texture live in ONE packed fp32 buffer, level l at offset off[l] (floats), holding bt x F x H_l x W_l x C
// (F = 6 faces for a cube map, 1 otherwise; bt = 1 is a texture broadcast over the lookup batch: its batch stride is 0, as tex_bstride in
// d3h_texture_fwd).  The level sizes come in as a HOST array lvl_hw[2 * nlev] = (H_0, W_0, H_1, W_1, ...).
#include "d3h_common.h"

#include <type_traits>

namespace {

constexpr int TEX_MAX_LEVELS = 16;
enum { TF_NEAREST = 0, TF_LINEAR = 1, TF_MIP_NEAREST = 2, TF_MIP_LINEAR = 3 };
enum { TB_WRAP = 0, TB_CLAMP = 1, TB_ZERO = 2, TB_CUBE = 3 };

struct TexLevels {
    int n, F, C;
    int H[TEX_MAX_LEVELS], W[TEX_MAX_LEVELS];
    long long off[TEX_MAX_LEVELS], bstride[TEX_MAX_LEVELS];
};

// fills the offsets / batch strides; false on a bad level list
static bool tex_levels(TexLevels& t, int bt, int faces, int C, int nlev, const int* lvl_hw) {
    if (bt <= 0 || (faces != 1 && faces != 6) || C <= 0 || nlev <= 0 || nlev > TEX_MAX_LEVELS || !lvl_hw) return false;
    t.n = nlev, t.F = faces, t.C = C;
    long long off = 0;
    for (int l = 0; l < nlev; ++l) {
        const int h = lvl_hw[2 * l], w = lvl_hw[2 * l + 1];
        if (h <= 0 || w <= 0 || (faces == 6 && h != w)) return false;
        const long long per_b = (long long)faces * h * w * C;
        t.H[l] = h, t.W[l] = w, t.off[l] = off, t.bstride[l] = bt > 1 ? per_b : 0;
        off += per_b * bt;
    }
    return true;
}

// float -> int tap coordinate that is safe for any input (NaN and huge values included): every boundary mode then maps it into range
__device__ __forceinline__ float tex_sane(float x) { return fminf(fmaxf(x, -1.0e8f), 1.0e8f); }

template <int BND>
__device__ __forceinline__ int tex_bound(int i, int n, bool& ok) {
    if (BND == TB_WRAP) return ((i % n) + n) % n;
    if (BND == TB_ZERO) { ok = ok && i >= 0 && i < n; return min(max(i, 0), n - 1); }
    return min(max(i, 0), n - 1);                         // clamp (a cube tap that leaves its face is re-resolved before this)
}

// ---- cube maps: faces +x, -x, +y, -y, +z, -z.  x along W, y along H, both in [-1, 1] at the face edges; the inverse of
// render/util.py:cube_to_dir.  A face's (x, y) are (sA * d[A] / |d[M]|, sB * d[B] / |d[M]|) for its major axis M.
__device__ __forceinline__ void cube_face_axes(int s, int& A, float& sA, int& Bx, float& sB) {
    switch (s) {
        case 0: A = 2, sA = -1.f, Bx = 1, sB = -1.f; break;
        case 1: A = 2, sA = 1.f, Bx = 1, sB = -1.f; break;
        case 2: A = 0, sA = 1.f, Bx = 2, sB = 1.f; break;
        case 3: A = 0, sA = 1.f, Bx = 2, sB = -1.f; break;
        case 4: A = 0, sA = 1.f, Bx = 1, sB = -1.f; break;
        default: A = 0, sA = -1.f, Bx = 1, sB = -1.f; break;
    }
}

// major axis (ties: x before y before z) -> face, face coordinates in [-1, 1]
__device__ __forceinline__ int cube_face(const float d[3], float& x, float& y) {
    const float ax = fabsf(d[0]), ay = fabsf(d[1]), az = fabsf(d[2]);
    const int M = (ax >= ay && ax >= az) ? 0 : (ay >= az ? 1 : 2);
    const int s = 2 * M + (d[M] < 0.f ? 1 : 0);
    int A, Bx;
    float sA, sB;
    cube_face_axes(s, A, sA, Bx, sB);
    const float m = fabsf(d[M]);
    x = sA * d[A] / m, y = sB * d[Bx] / m;
    return s;
}

__device__ __forceinline__ void cube_dir(int s, float x, float y, float d[3]) {
    switch (s) {
        case 0: d[0] = 1.f, d[1] = -y, d[2] = -x; break;
        case 1: d[0] = -1.f, d[1] = -y, d[2] = x; break;
        case 2: d[0] = x, d[1] = 1.f, d[2] = y; break;
        case 3: d[0] = x, d[1] = -1.f, d[2] = -y; break;
        case 4: d[0] = x, d[1] = -y, d[2] = 1.f; break;
        default: d[0] = -x, d[1] = -y, d[2] = -1.f; break;
    }
}

// The (up to) four taps of one lookup into one level: element offsets (of channel 0), validity, and the bilinear fractions.  corner >= 0:
// that tap of a cube lookup left its face across two edges; its value is the average of the other three taps.
struct Taps {
    long long off[4];
    bool ok[4];
    float fx, fy;
    int corner;
};

// 2-D: (u, v); cube: the direction.  px / py: d(texel x, y)/d(uv) -- 2-D: W_l, H_l; cube: a 3-vector each (the face projection).
template <bool NEAREST, int BND>
__device__ __forceinline__ void tex_taps(const TexLevels& T, int l, int b, const float* uvp, Taps& tp, float px[3], float py[3]) {
    const int h = T.H[l], w = T.W[l], C = T.C;
    const long long base = T.off[l] + (long long)b * T.bstride[l];
    tp.corner = -1;
    if (BND != TB_CUBE) {
        const float X = tex_sane(uvp[0] * w - (NEAREST ? 0.f : 0.5f)), Y = tex_sane(uvp[1] * h - (NEAREST ? 0.f : 0.5f));
        const float xf = floorf(X), yf = floorf(Y);
        tp.fx = NEAREST ? 0.f : X - xf, tp.fy = NEAREST ? 0.f : Y - yf;
        px[0] = (float)w, px[1] = 0.f, py[0] = 0.f, py[1] = (float)h;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            bool ok = true;
            const int ix = tex_bound<BND>((int)xf + (k & 1), w, ok), iy = tex_bound<BND>((int)yf + (k >> 1), h, ok);
            tp.ok[k] = ok && (!NEAREST || k == 0);
            tp.off[k] = base + ((long long)iy * w + ix) * C;
        }
        return;
    }
    const int n = w;
    float d[3] = {uvp[0], uvp[1], uvp[2]}, x, y;
    const int s = cube_face(d, x, y);
    const float X = tex_sane((x + 1.f) * 0.5f * n - (NEAREST ? 0.f : 0.5f)), Y = tex_sane((y + 1.f) * 0.5f * n - (NEAREST ? 0.f : 0.5f));
    const float xf = floorf(X), yf = floorf(Y);
    tp.fx = NEAREST ? 0.f : X - xf, tp.fy = NEAREST ? 0.f : Y - yf;
    {   // d(X)/d(dir), d(Y)/d(dir)
        int A, Bx;
        float sA, sB;
        cube_face_axes(s, A, sA, Bx, sB);
        const int M = s >> 1;
        const float m = fabsf(d[M]), hn = 0.5f * n;
        px[0] = px[1] = px[2] = py[0] = py[1] = py[2] = 0.f;
        px[A] = hn * sA / m, px[M] = -hn * x / d[M];
        py[Bx] = hn * sB / m, py[M] = -hn * y / d[M];
        if (!(m > 0.f)) px[0] = px[1] = px[2] = py[0] = py[1] = py[2] = 0.f;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        int ix = (int)xf + (k & 1), iy = (int)yf + (k >> 1), fs = s;
        const bool outx = !NEAREST && (ix < 0 || ix >= n), outy = !NEAREST && (iy < 0 || iy >= n);     // nearest: the face's own texel, clamped
        tp.ok[k] = !NEAREST || k == 0;
        if (outx && outy) {
            tp.corner = k, tp.ok[k] = false;
        } else if (outx || outy) {              // the adjacent face's texel in the direction of this tap's centre
            float td[3], tx, ty;
            cube_dir(s, (2.f * ix + 1.f) / n - 1.f, (2.f * iy + 1.f) / n - 1.f, td);
            fs = cube_face(td, tx, ty);
            ix = (int)floorf(tex_sane((tx + 1.f) * 0.5f * n)), iy = (int)floorf(tex_sane((ty + 1.f) * 0.5f * n));
        }
        ix = min(max(ix, 0), n - 1), iy = min(max(iy, 0), n - 1);
        tp.off[k] = base + (((long long)fs * n + iy) * n + ix) * C;
    }
}

template <int VW>
__device__ __forceinline__ void ldv(const float* p, float* v) {
    if constexpr (VW == 4) {
        const float4 q = *reinterpret_cast<const float4*>(p);
        v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
    } else {
        v[0] = *p;
    }
}

// the four tap values of one channel chunk (corner of a cube lookup: the mean of the other three)
template <int VW>
__device__ __forceinline__ void tap_values(const float* __restrict__ tex, const Taps& tp, int c, float t[4][VW]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (tp.ok[k]) ldv<VW>(tex + tp.off[k] + c, t[k]);
        else
#pragma unroll
            for (int j = 0; j < VW; ++j) t[k][j] = 0.f;
    }
    if (tp.corner >= 0) {
        const int q = tp.corner;
#pragma unroll
        for (int j = 0; j < VW; ++j) t[q][j] = (t[0][j] + t[1][j] + t[2][j] + t[3][j]) * (1.f / 3.f);
    }
}

// mip level of one pixel: 0.5 log2(lambda) + bias clamped to [0, L-1]; dl_da / dl_db: its derivatives (0 where clamped, or lambda = 0)
__device__ __forceinline__ float tex_lod(const TexLevels& T, const float* __restrict__ uv_da, const float* __restrict__ bias, size_t i, float dl_da[4],
                                         float& dl_db) {
    float lev = 0.f, g_lam = 0.f;
    dl_da[0] = dl_da[1] = dl_da[2] = dl_da[3] = 0.f;
    dl_db = bias ? 1.f : 0.f;
    float a = 0.f, b = 0.f, c = 0.f, d = 0.f, A = 0.f, D = 0.f, B = 0.f, r = 0.f;
    if (uv_da) {
        a = uv_da[4 * i + 0] * T.W[0], b = uv_da[4 * i + 1] * T.W[0], c = uv_da[4 * i + 2] * T.H[0], d = uv_da[4 * i + 3] * T.H[0];
        A = a * a + c * c, D = b * b + d * d, B = a * b + c * d;
        const float hd = 0.5f * (A - D);
        r = sqrtf(hd * hd + B * B);
        const float lam = 0.5f * (A + D) + r;
        if (!(lam > 0.f)) { dl_db = 0.f; return 0.f; }
        lev = 0.5f * log2f(lam);
        g_lam = 0.5f / (lam * 0.69314718055994531f);
    }
    if (bias) lev += bias[i];
    const float top = (float)(T.n - 1);
    if (!(lev > 0.f) || lev > top) {                       // clamped (NaN included): no gradient
        dl_db = 0.f;
        return lev > top ? top : 0.f;
    }
    if (uv_da) {
        const float dA = r > 0.f ? 0.5f + 0.25f * (A - D) / r : 0.5f, dD = r > 0.f ? 0.5f - 0.25f * (A - D) / r : 0.5f, dB = r > 0.f ? B / r : 0.f;
        // d lambda / d(a, b, c, d), then the W0 / H0 scale of a, b (u) and c, d (v)
        dl_da[0] = g_lam * (dA * 2.f * a + dB * b) * T.W[0];
        dl_da[1] = g_lam * (dD * 2.f * b + dB * a) * T.W[0];
        dl_da[2] = g_lam * (dA * 2.f * c + dB * d) * T.H[0];
        dl_da[3] = g_lam * (dD * 2.f * d + dB * c) * T.H[0];
    }
    return lev;
}

// the levels a pixel reads and their blend weights (w1 = 0: one level)
template <int FILT>
__device__ __forceinline__ void tex_pick(const TexLevels& T, float lev, int& l0, int& l1, float& w1) {
    l0 = 0, l1 = 0, w1 = 0.f;
    if (FILT == TF_MIP_NEAREST) {
        l0 = l1 = min(max((int)floorf(lev + 0.5f), 0), T.n - 1);
    } else if (FILT == TF_MIP_LINEAR) {
        l0 = min((int)floorf(lev), T.n - 1);
        w1 = lev - (float)l0;
        l1 = min(l0 + 1, T.n - 1);
        if (l1 == l0) w1 = 0.f;
    }
}

// One lane per output pixel.  2-D uv: 2 floats / pixel, cube: 3.
template <int FILT, int BND, int VW>
__global__ __launch_bounds__(256) void texlookup_fwd_kernel(const float* __restrict__ tex, TexLevels T, const float* __restrict__ uv,
                                                            const float* __restrict__ uv_da, const float* __restrict__ bias, size_t n, size_t npb,
                                                            float* __restrict__ out) {
    constexpr bool NEAREST = FILT == TF_NEAREST;
    constexpr bool MIP = FILT == TF_MIP_NEAREST || FILT == TF_MIP_LINEAR;
    constexpr int UVW = BND == TB_CUBE ? 3 : 2;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int b = (int)(i / npb), C = T.C;
    int l0 = 0, l1 = 0;
    float w1 = 0.f;
    if (MIP) {
        float dl[4], dlb;
        tex_pick<FILT>(T, tex_lod(T, uv_da, bias, i, dl, dlb), l0, l1, w1);
    }
    Taps t0, t1;
    float px[3], py[3];
    tex_taps<NEAREST, BND>(T, l0, b, uv + UVW * i, t0, px, py);
    if (FILT == TF_MIP_LINEAR) tex_taps<false, BND>(T, l1, b, uv + UVW * i, t1, px, py);
    for (int c = 0; c < C; c += VW) {
        float t[4][VW], o[VW];
        tap_values<VW>(tex, t0, c, t);
#pragma unroll
        for (int j = 0; j < VW; ++j)
            o[j] = (t[0][j] * (1.f - t0.fx) + t[1][j] * t0.fx) * (1.f - t0.fy) + (t[2][j] * (1.f - t0.fx) + t[3][j] * t0.fx) * t0.fy;
        if (FILT == TF_MIP_LINEAR && w1 != 0.f) {
            tap_values<VW>(tex, t1, c, t);
#pragma unroll
            for (int j = 0; j < VW; ++j) {
                const float o1 = (t[0][j] * (1.f - t1.fx) + t[1][j] * t1.fx) * (1.f - t1.fy) + (t[2][j] * (1.f - t1.fx) + t[3][j] * t1.fx) * t1.fy;
                o[j] = o[j] * (1.f - w1) + o1 * w1;
            }
        }
#pragma unroll
        for (int j = 0; j < VW; ++j) out[i * C + c + j] = o[j];
    }
}

// g: the output gradient of one level's bilinear value (already scaled by that level's blend weight).  Scatters into d_tex, returns
// d(value)/d(fx), d(value)/d(fy) (accumulated into gfx, gfy) and the level's value (for the blend weight's gradient) into val.
template <int VW>
__device__ __forceinline__ void level_bwd(const float* __restrict__ tex, float* __restrict__ d_tex, const Taps& tp, int c, const float* g,
                                          float scale, bool need_tex, bool need_val, float& gfx, float& gfy, float* val) {
    const float wk[4] = {(1.f - tp.fx) * (1.f - tp.fy), tp.fx * (1.f - tp.fy), (1.f - tp.fx) * tp.fy, tp.fx * tp.fy};
    if (need_tex) {
        float w[4] = {wk[0], wk[1], wk[2], wk[3]};
        if (tp.corner >= 0) {
            const float s = w[tp.corner] * (1.f / 3.f);
            w[tp.corner] = 0.f;
#pragma unroll
            for (int k = 0; k < 4; ++k) w[k] += s;
            w[tp.corner] = 0.f;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (!tp.ok[k] || w[k] == 0.f) continue;
#pragma unroll
            for (int j = 0; j < VW; ++j)
                if (g[j] != 0.f) atomicAdd(d_tex + tp.off[k] + c + j, g[j] * scale * w[k]);
        }
    }
    if (need_val) {
        float t[4][VW];
        tap_values<VW>(tex, tp, c, t);
#pragma unroll
        for (int j = 0; j < VW; ++j) {
            gfx += g[j] * scale * ((t[1][j] - t[0][j]) * (1.f - tp.fy) + (t[3][j] - t[2][j]) * tp.fy);
            gfy += g[j] * scale * ((t[2][j] - t[0][j]) * (1.f - tp.fx) + (t[3][j] - t[1][j]) * tp.fx);
            val[j] = (t[0][j] * wk[0] + t[1][j] * wk[1]) + (t[2][j] * wk[2] + t[3][j] * wk[3]);
        }
    }
}

// d_tex: accumulated with fp32 atomics into the packed level buffer (caller zero-fills).  d_uv, d_uv_da, d_bias: overwritten, one lane per
// pixel, no atomics; each may be NULL.
template <int FILT, int BND, int VW>
__global__ __launch_bounds__(256) void texlookup_bwd_kernel(const float* __restrict__ tex, TexLevels T, const float* __restrict__ uv,
                                                            const float* __restrict__ uv_da, const float* __restrict__ bias, size_t n, size_t npb,
                                                            const float* __restrict__ g_out, float* __restrict__ d_tex, float* __restrict__ d_uv,
                                                            float* __restrict__ d_uv_da, float* __restrict__ d_bias) {
    constexpr bool NEAREST = FILT == TF_NEAREST;
    constexpr bool MIP = FILT == TF_MIP_NEAREST || FILT == TF_MIP_LINEAR;
    constexpr int UVW = BND == TB_CUBE ? 3 : 2;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int b = (int)(i / npb), C = T.C;
    int l0 = 0, l1 = 0;
    float w1 = 0.f, dl[4] = {0.f, 0.f, 0.f, 0.f}, dlb = 0.f;
    if (MIP) tex_pick<FILT>(T, tex_lod(T, uv_da, bias, i, dl, dlb), l0, l1, w1);
    const bool two = FILT == TF_MIP_LINEAR && w1 != 0.f;
    Taps t0, t1;
    float px0[3], py0[3], px1[3], py1[3];
    tex_taps<NEAREST, BND>(T, l0, b, uv + UVW * i, t0, px0, py0);
    if (two) tex_taps<false, BND>(T, l1, b, uv + UVW * i, t1, px1, py1);
    const bool need_uv = d_uv && !NEAREST;
    const bool need_lev = FILT == TF_MIP_LINEAR && (d_uv_da || d_bias);
    float gfx0 = 0.f, gfy0 = 0.f, gfx1 = 0.f, gfy1 = 0.f, glev = 0.f;
    for (int c = 0; c < C; c += VW) {
        float g[VW], v0[VW], v1[VW];
        ldv<VW>(g_out + i * C + c, g);
        level_bwd<VW>(tex, d_tex, t0, c, g, two ? 1.f - w1 : 1.f, d_tex != nullptr, need_uv || (two && need_lev), gfx0, gfy0, v0);
        if (two) {
            level_bwd<VW>(tex, d_tex, t1, c, g, w1, d_tex != nullptr, true, gfx1, gfy1, v1);
#pragma unroll
            for (int j = 0; j < VW; ++j) glev += g[j] * (v1[j] - v0[j]);
        }
    }
    if (d_uv) {
#pragma unroll
        for (int k = 0; k < UVW; ++k) {
            float s = NEAREST ? 0.f : gfx0 * px0[k] + gfy0 * py0[k];
            if (two) s += gfx1 * px1[k] + gfy1 * py1[k];
            d_uv[UVW * i + k] = s;
        }
    }
    if (d_uv_da)
#pragma unroll
        for (int k = 0; k < 4; ++k) d_uv_da[4 * i + k] = glev * dl[k];
    if (d_bias) d_bias[i] = glev * dlb;
}

// ---- pyramid ---------------------------------------------------------------------------------------------------------------------------
// level l from level l - 1: the 2 x 2 box average (a dimension of 1 stays 1 and averages over the other one only).  One lane per texel.
__global__ __launch_bounds__(256) void texmip_down_kernel(float* __restrict__ pyr, TexLevels T, int l, int bt) {
    const int hc = T.H[l], wc = T.W[l], hp = T.H[l - 1], wp = T.W[l - 1], C = T.C;
    const size_t n = (size_t)bt * T.F * hc * wc;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int x = (int)(i % wc), y = (int)((i / wc) % hc);
    const size_t img = i / ((size_t)wc * hc);                       // (batch, face)
    const int sx = wp > wc ? 2 : 1, sy = hp > hc ? 2 : 1;
    const float wgt = 1.f / (sx * sy);
    const float* src = pyr + T.off[l - 1] + img * (size_t)hp * wp * C;
    float* dst = pyr + T.off[l] + i * C;
    for (int c = 0; c < C; ++c) {
        float s = 0.f;
        for (int dy = 0; dy < sy; ++dy)
            for (int dx = 0; dx < sx; ++dx) s += src[((size_t)(y * sy + dy) * wp + x * sx + dx) * C + c];
        dst[c] = s * wgt;
    }
}

// adjoint of the pyramid: each base texel gathers its ancestors' gradients times the product of the box weights on the way (4^-l while
// both dimensions halve).  Deterministic, no atomics.  g_tex overwritten.
__global__ __launch_bounds__(256) void texmip_bwd_kernel(const float* __restrict__ g_pyr, TexLevels T, int bt, float* __restrict__ g_tex) {
    const int h0 = T.H[0], w0 = T.W[0], C = T.C;
    const size_t n = (size_t)bt * T.F * h0 * w0;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int x0 = (int)(i % w0), y0 = (int)((i / w0) % h0);
    const size_t img = i / ((size_t)w0 * h0);
    for (int c = 0; c < C; ++c) {
        float s = g_pyr[i * C + c], wgt = 1.f;
        int x = x0, y = y0;
        for (int l = 1; l < T.n; ++l) {
            const int sx = T.W[l - 1] > T.W[l] ? 2 : 1, sy = T.H[l - 1] > T.H[l] ? 2 : 1;
            x /= sx, y /= sy, wgt *= 1.f / (sx * sy);
            s += wgt * g_pyr[T.off[l] + (img * T.H[l] * T.W[l] + (size_t)y * T.W[l] + x) * C + c];
        }
        g_tex[i * C + c] = s;
    }
}

template <int FILT, int BND, int VW>
static void launch_fwd(const float* tex, const TexLevels& T, const float* uv, const float* uv_da, const float* bias, size_t n, size_t npb, float* out,
                       hipStream_t s) {
    hipLaunchKernelGGL((texlookup_fwd_kernel<FILT, BND, VW>), dim3(d3h_cdiv(n, 256)), dim3(256), 0, s, tex, T, uv, uv_da, bias, n, npb, out);
}

template <int FILT, int BND, int VW>
static void launch_bwd(const float* tex, const TexLevels& T, const float* uv, const float* uv_da, const float* bias, size_t n, size_t npb,
                       const float* g_out, float* d_tex, float* d_uv, float* d_uv_da, float* d_bias, hipStream_t s) {
    hipLaunchKernelGGL((texlookup_bwd_kernel<FILT, BND, VW>), dim3(d3h_cdiv(n, 256)), dim3(256), 0, s, tex, T, uv, uv_da, bias, n, npb, g_out,
                       d_tex, d_uv, d_uv_da, d_bias);
}

// runtime (filter, boundary, channel-vector width) -> one template instance
template <class F>
static void tex_dispatch(int filter, int boundary, int vw, F&& f) {
#define D3H_TEX_VW(FI, BN) (vw == 4 ? f(std::integral_constant<int, FI>(), std::integral_constant<int, BN>(), std::integral_constant<int, 4>()) \
                                    : f(std::integral_constant<int, FI>(), std::integral_constant<int, BN>(), std::integral_constant<int, 1>()))
#define D3H_TEX_BND(FI)                         \
    switch (boundary) {                         \
        case TB_WRAP: D3H_TEX_VW(FI, TB_WRAP); break;   \
        case TB_CLAMP: D3H_TEX_VW(FI, TB_CLAMP); break; \
        case TB_ZERO: D3H_TEX_VW(FI, TB_ZERO); break;   \
        default: D3H_TEX_VW(FI, TB_CUBE); break;        \
    }
    switch (filter) {
        case TF_NEAREST: D3H_TEX_BND(TF_NEAREST); break;
        case TF_LINEAR: D3H_TEX_BND(TF_LINEAR); break;
        case TF_MIP_NEAREST: D3H_TEX_BND(TF_MIP_NEAREST); break;
        default: D3H_TEX_BND(TF_MIP_LINEAR); break;
    }
#undef D3H_TEX_BND
#undef D3H_TEX_VW
}

static bool tex_lookup_args(int bt, int nb, int H, int W, int filter, int boundary, const float* uv, const float* tex, int nlev) {
    if (nb <= 0 || H < 0 || W < 0 || filter < TF_NEAREST || filter > TF_MIP_LINEAR || boundary < TB_WRAP || boundary > TB_CUBE) return false;
    if (!uv || !tex || (bt != 1 && bt != nb)) return false;
    if ((filter == TF_NEAREST || filter == TF_LINEAR) && nlev != 1) return false;
    return true;
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------
// Mip pyramid, forward: pyr is the packed level buffer (layout: csrc/texture.hip header; lvl_hw HOST [nlev][2] = (H_l, W_l)); level 0 is in
// place, levels 1 .. nlev-1 are overwritten, each the 2 x 2 box average of the one above (a dimension of 1 stays 1, any other halves).
// bt = texture batch, faces = 1 (2-D) or 6 (cube, H_l = W_l).
extern "C" int d3h_texmip_build(float* pyr, int bt, int faces, int C, int nlev, const int* lvl_hw, void* stream) {
    TexLevels T;
    if (!pyr || !tex_levels(T, bt, faces, C, nlev, lvl_hw)) return D3H_ERR_ARG;
    for (int l = 1; l < nlev; ++l) {
        const bool okh = T.H[l] == (T.H[l - 1] == 1 ? 1 : T.H[l - 1] / 2) && (T.H[l - 1] == 1 || T.H[l - 1] % 2 == 0);
        const bool okw = T.W[l] == (T.W[l - 1] == 1 ? 1 : T.W[l - 1] / 2) && (T.W[l - 1] == 1 || T.W[l - 1] % 2 == 0);
        if (!okh || !okw) return D3H_ERR_ARG;
    }
    for (int l = 1; l < nlev; ++l) {
        const size_t n = (size_t)bt * faces * T.H[l] * T.W[l];
        hipLaunchKernelGGL(texmip_down_kernel, dim3(d3h_cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, pyr, T, l, bt);
    }
    D3H_LAUNCH_CHECK();
    return D3H_OK;
}

// Mip pyramid, backward: g_tex [bt][faces][H_0][W_0][C] (overwritten) = the gradient of level 0 plus every coarser level's gradient
// gathered down the pyramid (deterministic).
extern "C" int d3h_texmip_bwd(const float* g_pyr, float* g_tex, int bt, int faces, int C, int nlev, const int* lvl_hw, void* stream) {
    TexLevels T;
    if (!g_pyr || !g_tex || !tex_levels(T, bt, faces, C, nlev, lvl_hw)) return D3H_ERR_ARG;
    const size_t n = (size_t)bt * faces * T.H[0] * T.W[0];
    hipLaunchKernelGGL(texmip_bwd_kernel, dim3(d3h_cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, g_pyr, T, bt, g_tex);
    D3H_LAUNCH_CHECK();
    return D3H_OK;
}

// Texture lookup, forward.  pyr: packed levels (bt = 1 or nb); uv [nb][H][W][2] (boundary 3 = cube: [nb][H][W][3] directions);
// uv_da [nb][H][W][4] = (du/dX, du/dY, dv/dX, dv/dY) and bias [nb][H][W] (either may be NULL) drive the mip level of filters 2, 3.
// filter: 0 nearest, 1 linear, 2 linear-mipmap-nearest, 3 linear-mipmap-linear; boundary: 0 wrap, 1 clamp, 2 zero, 3 cube.
// out [nb][H][W][C] overwritten.
extern "C" int d3h_texlookup_fwd(const float* pyr, int bt, int C, int nlev, const int* lvl_hw, const float* uv, const float* uv_da,
                                 const float* bias, int nb, int H, int W, int filter, int boundary, float* out, void* stream) {
    TexLevels T;
    if (!out || !tex_lookup_args(bt, nb, H, W, filter, boundary, uv, pyr, nlev) || !tex_levels(T, bt, boundary == TB_CUBE ? 6 : 1, C, nlev, lvl_hw))
        return D3H_ERR_ARG;
    const size_t npb = (size_t)H * W, n = npb * nb;
    if (n == 0) return D3H_OK;
    tex_dispatch(filter, boundary, C % 4 == 0 ? 4 : 1, [&](auto fi, auto bn, auto vw) {
        launch_fwd<decltype(fi)::value, decltype(bn)::value, decltype(vw)::value>(pyr, T, uv, uv_da, bias, n, npb, out, (hipStream_t)stream);
    });
    D3H_LAUNCH_CHECK();
    return D3H_OK;
}

// Texture lookup, backward (arguments as the forward).  d_pyr: the packed levels' gradient, accumulated (caller zero-fills; NULL: not
// needed); d_uv [nb][H][W][2 or 3], d_uv_da [nb][H][W][4], d_bias [nb][H][W] overwritten (each may be NULL).
extern "C" int d3h_texlookup_bwd(const float* pyr, int bt, int C, int nlev, const int* lvl_hw, const float* uv, const float* uv_da,
                                 const float* bias, int nb, int H, int W, int filter, int boundary, const float* g_out, float* d_pyr, float* d_uv,
                                 float* d_uv_da, float* d_bias, void* stream) {
    TexLevels T;
    if (!g_out || !tex_lookup_args(bt, nb, H, W, filter, boundary, uv, pyr, nlev) ||
        !tex_levels(T, bt, boundary == TB_CUBE ? 6 : 1, C, nlev, lvl_hw) || (d_uv_da && !uv_da) || (d_bias && !bias))
        return D3H_ERR_ARG;
    const size_t npb = (size_t)H * W, n = npb * nb;
    if (n == 0) return D3H_OK;
    tex_dispatch(filter, boundary, C % 4 == 0 ? 4 : 1, [&](auto fi, auto bn, auto vw) {
        launch_bwd<decltype(fi)::value, decltype(bn)::value, decltype(vw)::value>(pyr, T, uv, uv_da, bias, n, npb, g_out, d_pyr, d_uv, d_uv_da,
                                                                                  d_bias, (hipStream_t)stream);
    });
    D3H_LAUNCH_CHECK();
    return D3H_OK;
}
