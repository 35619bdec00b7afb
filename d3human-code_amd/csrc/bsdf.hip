// bsdf.hip -- the per-pixel BSDF functions of render.renderutils on gfx950, forward and backward, one thread per pixel.
//
// Replaces (reference file:line): render/renderutils/c_src/bsdf.cu + torch_bindings.cpp (lambert, frostbite, pbr_specular, pbr_bsdf and the four
// test entry points fresnel_shlick / ndf_ggx / lambda_ggx / masking_smith).  The maths is that of the python twins, render/renderutils/bsdf.py:
// cosines clamped to [1e-4, 1 - 1e-4], alpha clamped to [min_roughness^2, 1], front-facing selects, F.normalize (x / max(|x|, 1e-12)).
// A clamp passes its gradient strictly inside its interval and a select passes none on the masked side, so masked pixels get exact zeros.
//
// Every input is [B,H,W,C] or broadcast along any of B / H / W (d3h_bcast.h).  The backward recomputes from the inputs (nothing else is
// saved), skips every gradient whose pointer is NULL, sums the gradient of an input that is broadcast along H and W inside the kernel, and
// writes the others at full resolution [B][H][W][C] (the wrapper sums those of inputs broadcast along one of the dims only).  These are
// streaming passes: <= 18 floats in, <= 18 out and O(100) flop per pixel.
#include "d3h_vec.h"
#include "d3h_bcast.h"
#include "d3h_bsdf_dev.h"

namespace {

enum { OP_SHLICK = 0, OP_NDF = 1, OP_LAMBDA = 2, OP_SMITH = 3, OP_LAMBERT = 4, OP_FROSTBITE = 5, OP_SPECULAR = 6, OP_PBR = 7, OP_COUNT = 8 };
constexpr int BSDF_MAX_IN = 6;
constexpr int OP_NIN[OP_COUNT] = {3, 2, 2, 3, 2, 4, 5, 6};      // number of inputs (their channel counts: d3h_bsdf_fwd below)

struct BsdfArgs {
    Bc in[BSDF_MAX_IN];
    float* d[BSDF_MAX_IN];      // backward: gradient of input k, or NULL (not wanted)
    int red[BSDF_MAX_IN];       // backward: 1 = input k is broadcast along H and W and d[k] is its [B or 1][C] sum (zero on entry), 0 = full resolution
    size_t npix;
    int H, W;
    float alpha_min;            // min_roughness^2
    int frostbite;              // pbr_bsdf: 0 lambert, 1 frostbite diffuse lobe
};

// ---- kernels --------------------------------------------------------------------------------------------------------------------
// Where gradient k goes.  Full resolution: one store per live pixel.  Reduced (the input is broadcast along H and W, e.g. view_pos [B,1,1,3],
// light_pos [1,1,1,3]): wave shuffles, then LDS, then one atomic per workgroup and channel into the [B or 1][C] sum -- at 1024^2 the
// full-resolution gradient plus torch's sum over it cost several times the kernel itself.  A workgroup whose pixels straddle two batch items
// (at most B - 1 of them) adds per pixel.  Every thread of the workgroup must call these (dead lanes pass live = false).
struct PutCtx { size_t i; bool live; int b; bool one_b; float* s4; };
__device__ __forceinline__ void put_n(const BsdfArgs& a, int k, const PutCtx& c, const float* v, int nch) {
    float* p = a.d[k];
    if (!p) return;
    if (!a.red[k]) {
        if (c.live) for (int ch = 0; ch < nch; ++ch) p[nch * c.i + ch] = v[ch];
        return;
    }
    float* q = p + (a.in[k].sb ? (size_t)c.b * nch : 0);
    if (c.one_b) {
        for (int ch = 0; ch < nch; ++ch) {
            float t = block_sum(c.live ? v[ch] : 0.f, c.s4);
            if (threadIdx.x == 0) atomicAdd(q + ch, t);
        }
    } else if (c.live) {
        for (int ch = 0; ch < nch; ++ch) atomicAdd(q + ch, v[ch]);
    }
}
__device__ __forceinline__ void put1(const BsdfArgs& a, int k, const PutCtx& c, float v) { put_n(a, k, c, &v, 1); }
__device__ __forceinline__ void put3(const BsdfArgs& a, int k, const PutCtx& c, V3 v) { float t[3] = {v.x, v.y, v.z}; put_n(a, k, c, t, 3); }

template <int OP>
__global__ __launch_bounds__(256) void bsdf_fwd_kernel(BsdfArgs a, float* __restrict__ out) {
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.npix) return;
    int b, y, x;
    bc_pixel(i, a.H, a.W, b, y, x);
#define IN3(k) fetch(a.in[k], b, y, x)
#define IN1(k) fetch1(a.in[k], b, y, x)
    if constexpr (OP == OP_SHLICK) {
        V3 f0 = IN3(0), f90 = IN3(1);
        float c = IN1(2);
        st3(out + 3 * i, mk(shlick_f(f0.x, f90.x, c), shlick_f(f0.y, f90.y, c), shlick_f(f0.z, f90.z, c)));
    } else if constexpr (OP == OP_NDF) {
        out[i] = ndf_f(IN1(0), IN1(1));
    } else if constexpr (OP == OP_LAMBDA) {
        out[i] = lambda_f(IN1(0), IN1(1));
    } else if constexpr (OP == OP_SMITH) {
        out[i] = smith_f(IN1(0), IN1(1), IN1(2));
    } else if constexpr (OP == OP_LAMBERT) {
        out[i] = lambert_f(IN3(0), IN3(1));
    } else if constexpr (OP == OP_FROSTBITE) {
        out[i] = frostbite_f(IN3(0), IN3(1), IN3(2), IN1(3));
    } else if constexpr (OP == OP_SPECULAR) {
        st3(out + 3 * i, specular_f(IN3(0), IN3(1), IN3(2), IN3(3), IN1(4), a.alpha_min));
    } else {
        V3 kd = IN3(0), arm = IN3(1), pos = IN3(2), n = IN3(3);
        V3 wo = fnormalize(IN3(4) - pos), wi = fnormalize(IN3(5) - pos);
        float spec = arm.x, rough = arm.y, metal = arm.z;
        float om = 1.0f - metal, os = 1.0f - spec;
        V3 ks = mk((0.04f * om + kd.x * metal) * os, (0.04f * om + kd.y * metal) * os, (0.04f * om + kd.z * metal) * os);
        float diff = a.frostbite ? frostbite_f(n, wi, wo, rough) : lambert_f(n, wi);
        st3(out + 3 * i, (kd * om) * diff + specular_f(ks, n, wo, wi, rough * rough, a.alpha_min));
    }
}

template <int OP>
__global__ __launch_bounds__(256) void bsdf_bwd_kernel(BsdfArgs a, const float* __restrict__ g_out) {
    __shared__ float s4[4];
    const size_t i0 = (size_t)blockIdx.x * 256, last = a.npix - 1;
    const bool live = i0 + threadIdx.x < a.npix;
    const size_t i = live ? i0 + threadIdx.x : last;         // dead lanes recompute the last pixel and store nothing: they only take part in the sums
    int b, y, x;
    bc_pixel(i, a.H, a.W, b, y, x);
    const size_t hw = (size_t)a.H * a.W;
    const PutCtx pc = {i, live, b, i0 / hw == (i0 + 255 < last ? i0 + 255 : last) / hw, s4};
    const V3 z3 = mk(0.f, 0.f, 0.f);
    if constexpr (OP == OP_SHLICK) {
        V3 f0 = IN3(0), f90 = IN3(1), g = ld3(g_out + 3 * i), d0 = z3, d1 = z3;
        float c = IN1(2), dc = 0.f;
        shlick_b(f0.x, f90.x, c, g.x, d0.x, d1.x, dc);
        shlick_b(f0.y, f90.y, c, g.y, d0.y, d1.y, dc);
        shlick_b(f0.z, f90.z, c, g.z, d0.z, d1.z, dc);
        put3(a, 0, pc, d0); put3(a, 1, pc, d1); put1(a, 2, pc, dc);
    } else if constexpr (OP == OP_NDF || OP == OP_LAMBDA) {
        float d0 = 0.f, d1 = 0.f;
        if (OP == OP_NDF) ndf_b(IN1(0), IN1(1), g_out[i], d0, d1);
        else lambda_b(IN1(0), IN1(1), g_out[i], d0, d1);
        put1(a, 0, pc, d0); put1(a, 1, pc, d1);
    } else if constexpr (OP == OP_SMITH) {
        float d0 = 0.f, d1 = 0.f, d2 = 0.f;
        smith_b(IN1(0), IN1(1), IN1(2), g_out[i], d0, d1, d2);
        put1(a, 0, pc, d0); put1(a, 1, pc, d1); put1(a, 2, pc, d2);
    } else if constexpr (OP == OP_LAMBERT) {
        V3 d0 = z3, d1 = z3;
        lambert_b(IN3(0), IN3(1), g_out[i], d0, d1);
        put3(a, 0, pc, d0); put3(a, 1, pc, d1);
    } else if constexpr (OP == OP_FROSTBITE) {
        V3 d0 = z3, d1 = z3, d2 = z3;
        float d3 = 0.f;
        frostbite_b(IN3(0), IN3(1), IN3(2), IN1(3), g_out[i], d0, d1, d2, d3);
        put3(a, 0, pc, d0); put3(a, 1, pc, d1); put3(a, 2, pc, d2); put1(a, 3, pc, d3);
    } else if constexpr (OP == OP_SPECULAR) {
        V3 d0 = z3, d1 = z3, d2 = z3, d3 = z3;
        float d4 = 0.f;
        specular_b(IN3(0), IN3(1), IN3(2), IN3(3), IN1(4), a.alpha_min, ld3(g_out + 3 * i), d0, d1, d2, d3, d4);
        put3(a, 0, pc, d0); put3(a, 1, pc, d1); put3(a, 2, pc, d2); put3(a, 3, pc, d3); put1(a, 4, pc, d4);
    } else {
        V3 kd = IN3(0), arm = IN3(1), pos = IN3(2), n = IN3(3), g = ld3(g_out + 3 * i);
        V3 wor = IN3(4) - pos, wir = IN3(5) - pos;
        V3 wo = fnormalize(wor), wi = fnormalize(wir);
        float spec = arm.x, rough = arm.y, metal = arm.z;
        float om = 1.0f - metal, os = 1.0f - spec;
        V3 kb = mk(0.04f * om + kd.x * metal, 0.04f * om + kd.y * metal, 0.04f * om + kd.z * metal);       // ks = kb (1 - spec)
        float diff = a.frostbite ? frostbite_f(n, wi, wo, rough) : lambert_f(n, wi);
        V3 g_n = z3, g_wo = z3, g_wi = z3, g_ks = z3;
        float g_rough = 0.f, g_alpha = 0.f;
        float g_diff = dot(g, kd) * om;
        if (a.frostbite) frostbite_b(n, wi, wo, rough, g_diff, g_n, g_wi, g_wo, g_rough);
        else lambert_b(n, wi, g_diff, g_n, g_wi);
        specular_b(kb * os, n, wo, wi, rough * rough, a.alpha_min, g, g_ks, g_n, g_wo, g_wi, g_alpha);
        g_rough += g_alpha * 2.0f * rough;
        V3 g_kd = g * (diff * om) + g_ks * (metal * os);
        float g_metal = -diff * dot(g, kd) + ((kd.x - 0.04f) * g_ks.x + (kd.y - 0.04f) * g_ks.y + (kd.z - 0.04f) * g_ks.z) * os;
        float g_spec = -dot(g_ks, kb);
        V3 g_view = fnormalize_bwd(wor, g_wo), g_light = fnormalize_bwd(wir, g_wi);
        put3(a, 0, pc, g_kd);
        put3(a, 1, pc, mk(g_spec, g_rough, g_metal));
        put3(a, 2, pc, (g_view + g_light) * -1.0f);
        put3(a, 3, pc, g_n);
        put3(a, 4, pc, g_view);
        put3(a, 5, pc, g_light);
    }
#undef IN3
#undef IN1
}

int bsdf_args(BsdfArgs& a, int op, int nin, const float* const* in, const int64_t* strides, int B, int H, int W, double min_roughness, int frostbite) {
    if (op < 0 || op >= OP_COUNT || nin != OP_NIN[op] || !in || !strides || B < 0 || H < 0 || W < 0) return D3H_ERR_ARG;
    for (int k = 0; k < BSDF_MAX_IN; ++k) {
        a.in[k] = k < nin ? bc_make(in[k], strides, k) : Bc{nullptr, 0, 0, 0};
        a.d[k] = nullptr;
        a.red[k] = 0;
        if (k < nin && !in[k]) return D3H_ERR_ARG;
    }
    a.npix = (size_t)B * H * W;
    a.H = H; a.W = W;
    a.alpha_min = (float)(min_roughness * min_roughness);
    a.frostbite = frostbite;
    return D3H_OK;
}

inline unsigned bsdf_blocks(size_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace

#define BSDF_DISPATCH(kernel, ...)                                                                                                \
    switch (op) {                                                                                                                 \
        case OP_SHLICK: hipLaunchKernelGGL(kernel<OP_SHLICK>, dim3(bsdf_blocks(a.npix)), dim3(256), 0, s, __VA_ARGS__); break;       \
        case OP_NDF: hipLaunchKernelGGL(kernel<OP_NDF>, dim3(bsdf_blocks(a.npix)), dim3(256), 0, s, __VA_ARGS__); break;             \
        case OP_LAMBDA: hipLaunchKernelGGL(kernel<OP_LAMBDA>, dim3(bsdf_blocks(a.npix)), dim3(256), 0, s, __VA_ARGS__); break;       \
        case OP_SMITH: hipLaunchKernelGGL(kernel<OP_SMITH>, dim3(bsdf_blocks(a.npix)), dim3(256), 0, s, __VA_ARGS__); break;         \
        case OP_LAMBERT: hipLaunchKernelGGL(kernel<OP_LAMBERT>, dim3(bsdf_blocks(a.npix)), dim3(256), 0, s, __VA_ARGS__); break;     \
        case OP_FROSTBITE: hipLaunchKernelGGL(kernel<OP_FROSTBITE>, dim3(bsdf_blocks(a.npix)), dim3(256), 0, s, __VA_ARGS__); break; \
        case OP_SPECULAR: hipLaunchKernelGGL(kernel<OP_SPECULAR>, dim3(bsdf_blocks(a.npix)), dim3(256), 0, s, __VA_ARGS__); break;   \
        default: hipLaunchKernelGGL(kernel<OP_PBR>, dim3(bsdf_blocks(a.npix)), dim3(256), 0, s, __VA_ARGS__); break;                 \
    }

// One per-pixel BSDF function.  op: 0 fresnel_shlick(f0[3], f90[3], cos[1]) -> [3]; 1 ndf_ggx(alphaSqr[1], cos[1]) -> [1]; 2 lambda_ggx(alphaSqr[1],
// cos[1]) -> [1]; 3 masking_smith(alphaSqr[1], cosI[1], cosO[1]) -> [1]; 4 lambert(nrm[3], wi[3]) -> [1]; 5 frostbite(nrm[3], wi[3], wo[3],
// linearRoughness[1]) -> [1]; 6 pbr_specular(col[3], nrm[3], wo[3], wi[3], alpha[1]) -> [3]; 7 pbr_bsdf(kd[3], arm[3], pos[3], nrm[3], view_pos[3],
// light_pos[3]) -> [3].  in: HOST array of the nin input pointers; strides: HOST [nin][3] element strides (b, h, w) of the inputs, 0 = broadcast;
// min_roughness: ops 6, 7; frostbite: op 7 (0 = lambert diffuse lobe).  out [B][H][W][channels] is overwritten.
extern "C" int d3h_bsdf_fwd(int op, int nin, const float* const* in, const int64_t* strides, int B, int H, int W, double min_roughness, int frostbite,
                            float* out, void* stream) {
    BsdfArgs a;
    if (bsdf_args(a, op, nin, in, strides, B, H, W, min_roughness, frostbite) != D3H_OK) return D3H_ERR_ARG;
    if (a.npix == 0) return D3H_OK;
    if (!out) return D3H_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    BSDF_DISPATCH(bsdf_fwd_kernel, a, out)
    D3H_LAUNCH_CHECK();
    return D3H_OK;
}
// Gradients of d3h_bsdf_fwd's inputs from g_out [B][H][W][channels of the output], recomputed from the inputs.  d_in: HOST array of nin
// pointers; d_in[k] [B][H][W][channels of input k] is overwritten at FULL resolution also where input k is broadcast (the caller sums), and
// skipped where d_in[k] is NULL.  reduce: NULL, or a HOST array of nin flags; reduce[k] = 1 (only for an input broadcast along H and W): d_in[k] is
// [B, or 1 if the input is broadcast along B as well][channels], ZERO on entry, and receives the gradient summed over H and W (float atomics, one
// per workgroup and channel: the last bits depend on their order).
extern "C" int d3h_bsdf_bwd(int op, int nin, const float* const* in, const int64_t* strides, int B, int H, int W, double min_roughness, int frostbite,
                            const float* g_out, float* const* d_in, const int* reduce, void* stream) {
    BsdfArgs a;
    if (bsdf_args(a, op, nin, in, strides, B, H, W, min_roughness, frostbite) != D3H_OK || !d_in) return D3H_ERR_ARG;
    if (a.npix == 0) return D3H_OK;
    if (!g_out) return D3H_ERR_ARG;
    for (int k = 0; k < nin; ++k) {
        a.d[k] = d_in[k];
        a.red[k] = reduce && reduce[k] ? 1 : 0;
        if (a.red[k] && (a.in[k].sh != 0 || a.in[k].sw != 0)) return D3H_ERR_ARG;
    }
    hipStream_t s = (hipStream_t)stream;
    BSDF_DISPATCH(bsdf_bwd_kernel, a, g_out)
    D3H_LAUNCH_CHECK();
    return D3H_OK;
}
