// texmat.hip -- the per-pixel material lookup of a textured mesh: raster -> texel coordinate -> up to three level-0 bilinear lookups, one pass.
//
// Replaces (reference file:line): render/render.py:277 (the interpolation of v_tex by t_tex_idx) followed by the three Texture2D.sample calls of
// the 2-D material branch of shade() (kd, ks, normal) for the case the exported atlas needs: level-0 bilinear, no uv gradient.  The composed
// route (d3h_interpolate_* + d3h_texlookup_*) stays the general one; this pass never stores the texel coordinate and reads the raster once.
//
// Conventions.  The texel coordinate is u t0 + v t1 + (1 - u - v) t2 of the triangle's three v_tex rows, summed in that order
// (interp_fwd_kernel of raster.hip).  The lookup is texture.hip's: texel centres at (i + 0.5) / N, u along W, v along H, the 2 x 2 texels
// around u W - 0.5 blended as (t00 (1 - fx) + t01 fx)(1 - fy) + (t10 (1 - fx) + t11 fx) fy; 'wrap' is the positive modulo of the tap
// index, 'clamp' clamps it.  A pixel with no triangle, with a triangle id above F or with a texture index outside [0, Vt) writes zeros and
// adds no gradient.  Maps of equal resolution share their taps and weights.
//
// Backward: one fp32 atomicAdd per tap and channel into the zero-filled gradient of each map that wants one (as texlookup_bwd_kernel); a
// zero product of weight and incoming gradient adds nothing.  The adds of a block's pixels are re-dealt to the lanes through LDS so that
// neighbouring lanes add to neighbouring floats, and a 1 x 1 map (a constant) is summed per wave first (see the kernel).  Not bitwise reproducible from run to run.  8 KiB of LDS, no scratch.
#include "d3h_common.h"

namespace {

constexpr int TM_T = 256;
constexpr int TM_MAPS = 3;
constexpr int TM_MAXC = 4;

struct TmMaps {
    const float* tex[TM_MAPS];     // [H][W][C]
    float* out[TM_MAPS];           // forward: [npix][C] (overwritten); backward: d_tex [H][W][C] (accumulated) or NULL
    const float* g[TM_MAPS];       // backward: the output gradient [npix][C]
    int H[TM_MAPS], W[TM_MAPS], C[TM_MAPS];
    int same[TM_MAPS];             // the first map of the same resolution (== its own index: compute the taps)
    int n;
};

struct TmTaps {
    int off[4];                    // texel index y W + x of the four taps
    float fx, fy;
};

__device__ __forceinline__ float tm_sane(float x) { return fminf(fmaxf(x, -1.0e8f), 1.0e8f); }

template <bool WRAP>
__device__ __forceinline__ int tm_bound(int i, int n) {
    if (WRAP) return ((i % n) + n) % n;
    return min(max(i, 0), n - 1);
}

template <bool WRAP>
__device__ __forceinline__ TmTaps tm_taps(float u, float v, int h, int w) {
    TmTaps tp;
    const float X = tm_sane(u * w - 0.5f), Y = tm_sane(v * h - 0.5f);
    const float xf = floorf(X), yf = floorf(Y);
    tp.fx = X - xf, tp.fy = Y - yf;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int ix = tm_bound<WRAP>((int)xf + (k & 1), w), iy = tm_bound<WRAP>((int)yf + (k >> 1), h);
        tp.off[k] = iy * w + ix;
    }
    return tp;
}

// the texel coordinate of pixel i; false: nothing to look up
__device__ __forceinline__ bool tm_texc(const float* __restrict__ rast, const float* __restrict__ v_tex, int64_t Vt, const int* __restrict__ tri, int64_t F,
                                        int64_t i, float& tu, float& tv) {
    const float4 r = *(const float4*)(rast + 4 * i);
    if (!(r.w >= 1.f) || r.w > (float)F) return false;               // NaN, empty, or an id past the face list
    const int64_t f = (int64_t)r.w - 1;
    if (f < 0 || f >= F) return false;
    const int64_t i0 = tri[3 * f], i1 = tri[3 * f + 1], i2 = tri[3 * f + 2];
    if (i0 < 0 || i0 >= Vt || i1 < 0 || i1 >= Vt || i2 < 0 || i2 >= Vt) return false;
    const float u = r.x, v = r.y, w = 1.0f - u - v;
    tu = u * v_tex[2 * i0] + v * v_tex[2 * i1] + w * v_tex[2 * i2];
    tv = u * v_tex[2 * i0 + 1] + v * v_tex[2 * i1 + 1] + w * v_tex[2 * i2 + 1];
    return true;
}

// the taps of map m: its own, or those of the earlier map of the same resolution
template <bool WRAP>
__device__ __forceinline__ TmTaps tm_taps_of(const TmMaps& M, int m, float tu, float tv, const TmTaps& t0, const TmTaps& t1) {
    if (m > 0 && M.same[m] == 0) return t0;
    if (m > 1 && M.same[m] == 1) return t1;
    return tm_taps<WRAP>(tu, tv, M.H[m], M.W[m]);
}

// one thread per pixel
template <bool WRAP>
__global__ __launch_bounds__(TM_T) void texmat_fwd_kernel(const float* __restrict__ rast, const float* __restrict__ v_tex, int64_t Vt,
                                                          const int* __restrict__ tri, int64_t F, int64_t npix, TmMaps M) {
    const int64_t i = (int64_t)blockIdx.x * TM_T + threadIdx.x;
    if (i >= npix) return;
    float tu = 0.f, tv = 0.f;
    const bool hit = tm_texc(rast, v_tex, Vt, tri, F, i, tu, tv);
    TmTaps t0 = {}, t1 = {};
#pragma unroll
    for (int m = 0; m < TM_MAPS; ++m) {
        if (m >= M.n) break;
        const int C = M.C[m];
        float* o = M.out[m] + i * C;
        if (!hit) {
            for (int c = 0; c < C; ++c) o[c] = 0.f;
            continue;
        }
        const TmTaps tp = tm_taps_of<WRAP>(M, m, tu, tv, t0, t1);
        if (m == 0) t0 = tp;
        if (m == 1) t1 = tp;
        const float* tex = M.tex[m];
        for (int c = 0; c < C; ++c) {
            const float a = tex[(int64_t)tp.off[0] * C + c], b = tex[(int64_t)tp.off[1] * C + c];
            const float d = tex[(int64_t)tp.off[2] * C + c], e = tex[(int64_t)tp.off[3] * C + c];
            o[c] = (a * (1.f - tp.fx) + b * tp.fx) * (1.f - tp.fy) + (d * (1.f - tp.fx) + e * tp.fx) * tp.fy;
        }
    }
}

// One block per TM_T pixels; M.out[m] is the gradient buffer of map m (NULL: that map wants none).  Per pixel and map the adds are 4 taps x C channels.
// A lane that kept its own pixel would send every one of them to an address of its own: 64 scattered 4-byte requests per wave-instruction, the
// slowest shape float atomics have.  So the taps and weights of the block's pixels go through LDS and the adds are dealt out again in the order
// (pixel, tap, channel): C consecutive lanes cover the C contiguous floats of one texel, and taps 0 / 1 (and 2 / 3) are neighbours along x, so a
// run of 2 C lanes usually covers 8 C contiguous bytes -- a wave-instruction touches about 64 / (2 C) segments instead of 64.
template <bool WRAP>
__global__ __launch_bounds__(TM_T) void texmat_bwd_kernel(const float* __restrict__ rast, const float* __restrict__ v_tex, int64_t Vt,
                                                          const int* __restrict__ tri, int64_t F, int64_t npix, TmMaps M) {
    __shared__ int s_off[TM_T][4];         // texel index of each tap; -1: no add from this pixel (empty, or past the image)
    __shared__ float s_w[TM_T][4];
    const int tid = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * TM_T;
    const int64_t i = base + tid;
    float tu = 0.f, tv = 0.f;
    const bool hit = i < npix && tm_texc(rast, v_tex, Vt, tri, F, i, tu, tv);
#pragma unroll
    for (int lead = 0; lead < TM_MAPS; ++lead) {
        if (lead >= M.n || M.same[lead] != lead) continue;            // (block-uniform)
        bool wanted = false;
        for (int m = lead; m < M.n; ++m) wanted = wanted || (M.same[m] == lead && M.out[m] != nullptr);
        if (!wanted) continue;
        __syncthreads();                                              // the previous resolution's taps have been consumed
        TmTaps tp = {};
        if (hit) tp = tm_taps<WRAP>(tu, tv, M.H[lead], M.W[lead]);
        const float w[4] = {(1.f - tp.fx) * (1.f - tp.fy), tp.fx * (1.f - tp.fy), (1.f - tp.fx) * tp.fy, tp.fx * tp.fy};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            s_off[tid][k] = hit ? tp.off[k] : -1;
            s_w[tid][k] = w[k];
        }
        __syncthreads();
        for (int m = lead; m < M.n; ++m) {
            float* d = M.out[m];
            if (M.same[m] != lead || !d) continue;
            const int C = M.C[m], per = 4 * C;
            const float* g = M.g[m] + base * C;
            if (M.H[m] == 1 && M.W[m] == 1) {
                // a constant: every add of the launch goes to the same C floats (the worst contention atomics have, and thousands of roundings in
                // arrival order).  Each wave sums its pixels first -- a fixed tree -- and adds once per channel.
                const float ws = hit ? (w[0] + w[1]) + (w[2] + w[3]) : 0.f;
                for (int c = 0; c < C; ++c) {
                    float v = hit ? g[tid * C + c] * ws : 0.f;
#pragma unroll
                    for (int sh = 32; sh > 0; sh >>= 1) v += __shfl_xor(v, sh);
                    if ((tid & 63) == 0 && v != 0.f) atomicAdd(d + c, v);
                }
                continue;
            }
            for (int j = tid; j < TM_T * per; j += TM_T) {
                const int p = j / per, r = j - p * per, k = r / C, c = r - k * C;
                const int off = s_off[p][k];
                if (off < 0) continue;
                const float val = g[p * C + c] * s_w[p][k];
                if (val != 0.f) atomicAdd(d + (int64_t)off * C + c, val);
            }
        }
    }
}

// argument checks shared by both directions; fills M (without out / g)
inline int tm_setup(const float* rast, const float* v_tex, int64_t Vt, const int* tri, int64_t F, int64_t npix, int n_maps, const void* const* tex,
                    const int* hwc, int boundary, TmMaps& M) {
    if (F < 0 || Vt < 0 || npix < 0 || n_maps < 1 || n_maps > TM_MAPS || !tex || !hwc || (boundary != 0 && boundary != 1)) return D3H_ERR_ARG;
    if (F > (1 << 24) || (npix + TM_T - 1) / TM_T > 0x7fffffff) return D3H_ERR_ARG;          // the raster stores the id as a float
    M.n = n_maps;
    for (int m = 0; m < TM_MAPS; ++m) {
        M.tex[m] = nullptr, M.out[m] = nullptr, M.g[m] = nullptr, M.H[m] = M.W[m] = M.C[m] = 1, M.same[m] = m;
        if (m >= n_maps) continue;
        const int h = hwc[3 * m], w = hwc[3 * m + 1], c = hwc[3 * m + 2];
        if (h < 1 || w < 1 || c < 1 || c > TM_MAXC || (int64_t)h * w > 0x7fffffff / TM_MAXC || !tex[m]) return D3H_ERR_ARG;
        M.tex[m] = (const float*)tex[m], M.H[m] = h, M.W[m] = w, M.C[m] = c;
        for (int q = m - 1; q >= 0; --q)
            if (M.H[q] == h && M.W[q] == w) M.same[m] = q;
    }
    if (npix > 0 && F > 0 && (!rast || !v_tex || !tri)) return D3H_ERR_ARG;
    if (npix > 0 && !rast) return D3H_ERR_ARG;
    if (((uintptr_t)rast & 15) != 0) return D3H_ERR_ARG;                                        // read as float4
    return D3H_OK;
}

}  // namespace

// Per-pixel material lookup, forward.  rast [npix][4] (u, v, _, triangle id + 1; 16-byte aligned), v_tex [Vt][2], tri [F][3] int32 rows of v_tex,
// n_maps in 1..3; tex and out are HOST arrays of n_maps device pointers, hwc a HOST array of n_maps (H, W, C) triples with C <= 4: map m is
// tex[m] [H][W][C], out[m] [npix][C] is overwritten with its level-0 bilinear value at the pixel's texel coordinate (boundary 0 wrap, 1 clamp), zeros
// where the pixel is empty.  One launch, one thread per pixel.  npix == 0 or F == 0 launches nothing (with F == 0 the caller zero-fills out).
extern "C" int d3h_texmat_fwd(const float* rast, const float* v_tex, int64_t Vt, const int* tri, int64_t F, int64_t npix, int n_maps,
                              const void* const* tex, const int* hwc, int boundary, void* const* out, void* stream) {
    TmMaps M;
    const int rc = tm_setup(rast, v_tex, Vt, tri, F, npix, n_maps, tex, hwc, boundary, M);
    if (rc != D3H_OK || !out) return D3H_ERR_ARG;
    for (int m = 0; m < n_maps; ++m) {
        if (!out[m] && npix > 0) return D3H_ERR_ARG;
        M.out[m] = (float*)out[m];
    }
    if (npix == 0 || F == 0) return D3H_OK;
    const dim3 grid((unsigned)((npix + TM_T - 1) / TM_T)), block(TM_T);
    if (boundary == 0)
        hipLaunchKernelGGL(texmat_fwd_kernel<true>, grid, block, 0, (hipStream_t)stream, rast, v_tex, Vt, tri, F, npix, M);
    else
        hipLaunchKernelGGL(texmat_fwd_kernel<false>, grid, block, 0, (hipStream_t)stream, rast, v_tex, Vt, tri, F, npix, M);
    D3H_LAUNCH_CHECK();
    return D3H_OK;
}

// Per-pixel material lookup, backward (arguments as d3h_texmat_fwd).  g_out is a HOST array of n_maps device pointers [npix][C] (the output gradients; may
// be NULL where d_tex[m] is), d_tex a HOST array of n_maps device pointers [H][W][C], ACCUMULATED with fp32 atomics (caller zero-fills); a NULL d_tex[m]
// means map m gets no gradient.  Nothing for empty pixels; no gradient to rast or v_tex.  One launch; npix == 0, F == 0 or all d_tex NULL launch nothing.
extern "C" int d3h_texmat_bwd(const float* rast, const float* v_tex, int64_t Vt, const int* tri, int64_t F, int64_t npix, int n_maps,
                              const void* const* tex, const int* hwc, int boundary, const void* const* g_out, void* const* d_tex, void* stream) {
    TmMaps M;
    const int rc = tm_setup(rast, v_tex, Vt, tri, F, npix, n_maps, tex, hwc, boundary, M);
    if (rc != D3H_OK || !g_out || !d_tex) return D3H_ERR_ARG;
    bool any = false;
    for (int m = 0; m < n_maps; ++m) {
        if (d_tex[m] && !g_out[m]) return D3H_ERR_ARG;
        M.out[m] = (float*)d_tex[m], M.g[m] = (const float*)g_out[m];
        any = any || d_tex[m] != nullptr;
    }
    if (npix == 0 || F == 0 || !any) return D3H_OK;
    const dim3 grid((unsigned)((npix + TM_T - 1) / TM_T)), block(TM_T);
    if (boundary == 0)
        hipLaunchKernelGGL(texmat_bwd_kernel<true>, grid, block, 0, (hipStream_t)stream, rast, v_tex, Vt, tri, F, npix, M);
    else
        hipLaunchKernelGGL(texmat_bwd_kernel<false>, grid, block, 0, (hipStream_t)stream, rast, v_tex, Vt, tri, F, npix, M);
    D3H_LAUNCH_CHECK();
    return D3H_OK;
}
