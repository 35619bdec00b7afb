// envshade.hip -- ray-traced shading under a lat-long environment light with multiple importance sampling, forward and backward, one thread
// per pixel; shadow rays go through the BVH of bvh.hip.
//
// Replaces (reference file:line): render/optixutils/c_src/envsampling/kernel.cu:463-542 (__raygen__rg with process_sample :403-461, the light
// probe functions :124-211 and the BSDF sampling :217-397), shaded with the module's own BSDF (c_src/bsdf.h: Lambert without albedo, GGX
// specular with min_roughness 0.08 and a specular colour that carries 1 - ks.x).  Per pixel with mask > 0: n^2 stratified samples of the light
// (inverse CDF over rows / cols[y]) and n^2 of the BSDF (cosine or GGX-VNDF lobe, chosen by pDiffuse), each weighted by the balance heuristic
// 1 / max(pdf_light + pdf_bsdf, 1e-4) and by the visibility V = occluded ? 1 - shadow_scale : 1.  Random numbers are the reference's PCG hash,
// seeded from (seed, linear pixel index), drawn in its order.  Sample directions, pdfs and visibility carry no gradient.  The backward re-runs
// the sampling with its own seed and recomputes everything; d(light) is a float atomicAdd per texel and channel, the rest plain stores.
#include "d3h_bsdf_dev.h"
#include "d3h_bvh_dev.h"

namespace {

constexpr float ES_MIN_ROUGHNESS = 0.08f;
constexpr float ES_ONE_BELOW = 0.99999994f;

struct EnvArgs {
    const float4* nodes; const float* tri9; int F;                  // the shadow-ray BVH (F = 0: nothing occludes)
    const float *mask, *ro, *pos, *nrm, *view, *kd, *ks;             // [B][H][W] / [B][H][W][3]
    const float* light; int LH, LW;                                  // [LH][LW][3]
    const float *pdf, *rows, *cols; int PH, PW;                      // [PH][PW], [PH], [PH][PW]
    const int* perms; int R;                                         // [R][n^2]
    size_t npix;
    int mode, n;                                                     // mode: 0 pbr, 1 diffuse, 2 white
    unsigned seed;
    float shadow_scale;
    float *diff, *spec;                                              // forward outputs [B][H][W][3]
    const float *g_diff, *g_spec;                                    // backward inputs
    float *d_pos, *d_nrm, *d_kd, *d_ks, *d_light;                    // backward outputs (d_pos, d_kd, d_ks may be NULL; d_light accumulated)
};

__device__ __forceinline__ unsigned rand_pcg(unsigned& state) {
    unsigned word = ((state >> ((state >> 28u) + 4u)) ^ state) * 277803737u;
    state = state * 747796405u + 2891336453u;
    return (word >> 22u) ^ word;
}
__device__ __forceinline__ float uniform_pcg(unsigned& state) { return (float)(rand_pcg(state) & 0xFFFFFFu) / (float)0x1000000; }

__device__ __forceinline__ V3 unit0(V3 v) {       // v / |v|, the zero vector stays zero
    float l = sqrtf(dot(v, v));
    return l > 0.0f ? v * (1.0f / l) : mk(0.f, 0.f, 0.f);
}
__device__ __forceinline__ float luminance(V3 c) { return c.x * 0.2126f + c.y * 0.7152f + c.z * 0.0722f; }

// Duff et al., "Building an orthonormal basis, revisited"
__device__ __forceinline__ void onb(V3 n, V3& b1, V3& b2) {
    float sign = copysignf(1.0f, n.z);
    float a = -1.0f / (sign + n.z);
    float b = n.x * n.y * a;
    b1 = mk(1.0f + sign * n.x * n.x * a, sign * b, -sign * n.x);
    b2 = mk(b, sign + n.y * n.y * a, -n.y);
}

// ---- the light probe ----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void dir_to_tc(V3 d, float& u, float& v) {
    u = atan2f(d.x, -d.z) / (2.0f * PI_F) + 0.5f;
    v = acosf(fminf(fmaxf(d.y, -1.0f), 1.0f)) / PI_F;
}
__device__ __forceinline__ int texel(float c, int size) {
    int i = (int)(c * (float)size);
    return i < 0 ? 0 : (i > size - 1 ? size - 1 : i);
}
// inverse CDF: idx = the first entry with x < cdf[idx] (the last one if there is none); returns the position inside that entry in [0, 1)
__device__ __forceinline__ float sample_cdf(const float* __restrict__ cdf, int size, float x, int& idx) {
    x = fminf(x, ES_ONE_BELOW);
    int lo = 0, hi = size - 1;
    while (lo < hi) {
        int mid = (lo + hi) >> 1;
        if (x < cdf[mid]) hi = mid; else lo = mid + 1;
    }
    idx = lo;
    float below = lo > 0 ? cdf[lo - 1] : 0.0f;
    return fminf((x - below) / (cdf[lo] - below), ES_ONE_BELOW);
}
__device__ __forceinline__ float light_pdf(const EnvArgs& a, V3 d) {
    float u, v;
    dir_to_tc(d, u, v);
    float w = (float)a.PH * (float)a.PW / (2.0f * PI_F * PI_F * fmaxf(sinf(v * PI_F), 0.0001f));
    return a.pdf[(size_t)texel(v, a.PH) * a.PW + texel(u, a.PW)] * w;
}
__device__ __forceinline__ V3 light_sample(const EnvArgs& a, float u, float v, float& pdf) {
    int x, y;
    float ry = sample_cdf(a.rows, a.PH, v, y);
    float rx = sample_cdf(a.cols + (size_t)y * a.PW, a.PW, u, x);
    float phi = (((float)x + rx) / (float)a.PW * 2.0f - 1.0f) * PI_F, theta = ((float)y + ry) / (float)a.PH * PI_F;
    float st = sinf(theta);
    V3 d = mk(st * sinf(phi), cosf(theta), -st * cosf(phi));
    pdf = light_pdf(a, d);
    return d;
}

// ---- BSDF sampling (local frame: z along the normal) -----------------------------------------------------------------------------------
__device__ __forceinline__ float g1_ggx(float a2, float c) {
    if (c <= 0.0f) return 0.0f;
    float c2 = c * c;
    return 2.0f / (1.0f + sqrtf(1.0f + a2 * (fmaxf(1.0f - c2, 0.0f) / c2)));
}
__device__ __forceinline__ float ndf_raw(float alpha, float c) {
    float a2 = alpha * alpha;
    float d = (c * a2 - c) * c + 1.0f;
    return a2 / (d * d * PI_F);
}
// pdf of the VNDF-sampled half vector h for the local view direction wo, over the reflection Jacobian
__device__ __forceinline__ float vndf_pdf(float alpha, V3 wo, V3 h) {
    float woH = dot(wo, h);
    return g1_ggx(alpha * alpha, wo.z) * ndf_raw(alpha, h.z) * fmaxf(0.0f, woH) / wo.z / (4.0f * woH);
}
__device__ __forceinline__ float ggx_pdf(V3 N, V3 wo, V3 wi, float alpha) {
    V3 W = unit0(N), U, V;
    onb(W, U, V);
    V3 wo_l = mk(dot(wo, U), dot(wo, V), dot(wo, W)), wi_l = mk(dot(wi, U), dot(wi, V), dot(wi, W));
    if (!(wo_l.z > 0.0f && wi_l.z > 0.0f)) return 0.0f;
    return vndf_pdf(alpha, wo_l, unit0(wi_l + wo_l));
}
// Heitz 2018, sampling the GGX distribution of visible normals
__device__ __forceinline__ V3 ggx_sample(V3 N, V3 wo, float ux, float uy, float alpha, float& pdf) {
    V3 W = unit0(N), U, V;
    onb(W, U, V);
    V3 wo_l = unit0(mk(dot(wo, U), dot(wo, V), dot(wo, W)));
    if (!(wo_l.z > 0.0f)) { pdf = 0.0f; return mk(0.f, 0.f, 0.f); }
    V3 Vh = unit0(mk(alpha * wo_l.x, alpha * wo_l.y, wo_l.z));
    V3 T1 = Vh.z < 0.9999f ? unit0(cross(mk(0.f, 0.f, 1.f), Vh)) : mk(1.f, 0.f, 0.f);
    V3 T2 = cross(Vh, T1);
    float r = sqrtf(ux), phi = (2.0f * PI_F) * uy;
    float t1 = r * cosf(phi), t2 = r * sinf(phi), s = 0.5f * (1.0f + Vh.z);
    t2 = (1.0f - s) * sqrtf(1.0f - t1 * t1) + s * t2;
    V3 Nh = T1 * t1 + T2 * t2 + Vh * sqrtf(fmaxf(0.0f, 1.0f - t1 * t1 - t2 * t2));
    V3 h = unit0(mk(alpha * Nh.x, alpha * Nh.y, fmaxf(0.0f, Nh.z)));
    pdf = vndf_pdf(alpha, wo_l, h);
    V3 wi_l = h * (dot(wo_l, h) * 2.0f) - wo_l;
    return unit0(U * wi_l.x + V * wi_l.y + W * wi_l.z);
}
__device__ __forceinline__ V3 cosine_sample(V3 N, float u, float v, float& pdf) {
    V3 W = unit0(N), U, V;
    onb(W, U, V);
    float phi = 2.0f * PI_F * u, ct = sqrtf(v), st = sqrtf(1.0f - v);
    pdf = fmaxf(0.000001f, ct / PI_F);
    return unit0(U * (cosf(phi) * st) + V * (sinf(phi) * st) + W * ct);
}
__device__ __forceinline__ void add_pdf(float& pdf, float other, float weight) {
    if (weight > 0.000001f) pdf += other * weight;
}
// one direction from the lobe chosen by s.z against pDiffuse; pdf: that of the mixture
__device__ __forceinline__ V3 bsdf_sample(float pD, float pS, V3 N, V3 wo, V3 s, float alpha, float& pdf, bool& diffuse_lobe) {
    pdf = 0.0f;
    diffuse_lobe = s.z < pD;
    V3 wi;
    if (diffuse_lobe) {
        if (pD < 0.0001f) { pdf = 1.0f; return N; }
        wi = cosine_sample(N, s.x, s.y, pdf);
        pdf *= pD;
        if (pS > 0.0f) add_pdf(pdf, ggx_pdf(N, wo, wi, alpha), 1.0f - pD);
    } else {
        wi = ggx_sample(N, wo, s.x, s.y, alpha, pdf);
        pdf *= 1.0f - pD;
        if (pD > 0.0f) add_pdf(pdf, fmaxf(dot(N, wi), 0.0f) / PI_F, pD);
    }
    return wi;
}
__device__ __forceinline__ float bsdf_pdf(float pD, float pS, V3 N, V3 wo, V3 wi, float alpha) {
    if (fminf(dot(N, wo), dot(N, wi)) < 1e-6f) return 1.0f;
    float pdf = 0.0f;
    if (pD > 0.0f) add_pdf(pdf, fmaxf(dot(N, wi), 0.0f) / PI_F, pD);
    if (pS > 0.0f) add_pdf(pdf, ggx_pdf(N, wo, wi, alpha), 1.0f - pD);
    return pdf;
}

// ---- one pixel ------------------------------------------------------------------------------------------------------------------------
struct Pixel {
    V3 ro, pos, nrm, view, kd, ks, wo, kb;      // kb: specular colour before its (1 - ks.x)
    V3 g_diff, g_spec;                            // backward: incoming gradients
    V3 acc_diff, acc_spec;                        // forward: sums
    V3 d_nrm, d_kd, d_ks, d_wo;                   // backward: sums
};

template <bool BWD>
__device__ __forceinline__ void shade_sample(const EnvArgs& a, Pixel& p, V3 wi, float pdf_sum, float frac) {
    float u, v;
    dir_to_tc(wi, u, v);
    const size_t tex = 3 * ((size_t)texel(v, a.LH) * a.LW + texel(u, a.LW));
    const V3 L = ld3(a.light + tex);
    const float mis = 1.0f / fmaxf(pdf_sum, 0.0001f);
    const float alpha = p.ks.y * p.ks.y, amin = ES_MIN_ROUGHNESS * ES_MIN_ROUGHNESS;
    const float fd = lambert_f(p.nrm, wi);
    const V3 fs = a.mode == 0 ? specular_f(p.kb * (1.0f - p.ks.x), p.nrm, p.wo, wi, alpha, amin) : mk(0.f, 0.f, 0.f);
    const bool hit = bvh_any_hit(a.nodes, a.tri9, a.F, p.ro, wi, 0.0f, 1e16f);
    const float w = (hit ? 1.0f - a.shadow_scale : 1.0f) * mis * frac;
    if (!BWD) {
        p.acc_diff = p.acc_diff + L * (fd * w);
        p.acc_spec = p.acc_spec + mk(fs.x * L.x, fs.y * L.y, fs.z * L.z) * w;
        return;
    }
    atomicAdd(a.d_light + tex, (p.g_diff.x * fd + p.g_spec.x * fs.x) * w);
    atomicAdd(a.d_light + tex + 1, (p.g_diff.y * fd + p.g_spec.y * fs.y) * w);
    atomicAdd(a.d_light + tex + 2, (p.g_diff.z * fd + p.g_spec.z * fs.z) * w);
    const V3 gd = mk(p.g_diff.x * L.x, p.g_diff.y * L.y, p.g_diff.z * L.z) * w, gs = mk(p.g_spec.x * L.x, p.g_spec.y * L.y, p.g_spec.z * L.z) * w;
    V3 d_wi = mk(0.f, 0.f, 0.f);
    lambert_b(p.nrm, wi, gd.x + gd.y + gd.z, p.d_nrm, d_wi);
    if (a.mode == 0) {
        V3 d_col = mk(0.f, 0.f, 0.f);
        float d_alpha = 0.0f;
        specular_b(p.kb * (1.0f - p.ks.x), p.nrm, p.wo, wi, alpha, amin, gs, d_col, p.d_nrm, p.d_wo, d_wi, d_alpha);
        const float os = 1.0f - p.ks.x, metal = p.ks.z;
        p.d_kd = p.d_kd + d_col * (metal * os);
        p.d_ks.x -= dot(d_col, p.kb);
        p.d_ks.y += d_alpha * 2.0f * p.ks.y;
        p.d_ks.z += ((p.kd.x - 0.04f) * d_col.x + (p.kd.y - 0.04f) * d_col.y + (p.kd.z - 0.04f) * d_col.z) * os;
    }
}

template <bool BWD>
__global__ __launch_bounds__(256) void env_shade_kernel(EnvArgs a) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.npix) return;
    const V3 z3 = mk(0.f, 0.f, 0.f);
    if (!(a.mask[i] > 0.0f)) {
        if (!BWD) { st3(a.diff + 3 * i, z3); st3(a.spec + 3 * i, z3); }
        else {
            st3(a.d_nrm + 3 * i, z3);
            if (a.d_pos) st3(a.d_pos + 3 * i, z3);
            if (a.d_kd) st3(a.d_kd + 3 * i, z3);
            if (a.d_ks) st3(a.d_ks + 3 * i, z3);
        }
        return;
    }
    Pixel p;
    p.ro = ld3(a.ro + 3 * i); p.pos = ld3(a.pos + 3 * i); p.nrm = ld3(a.nrm + 3 * i); p.view = ld3(a.view + 3 * i);
    p.kd = ld3(a.kd + 3 * i); p.ks = ld3(a.ks + 3 * i);
    p.g_diff = BWD ? ld3(a.g_diff + 3 * i) : z3;
    p.g_spec = BWD ? ld3(a.g_spec + 3 * i) : z3;
    p.acc_diff = p.acc_spec = p.d_nrm = p.d_kd = p.d_ks = p.d_wo = z3;
    const V3 wor = p.view - p.pos;
    p.wo = unit0(wor);
    const float metal = p.ks.z, alpha = p.ks.y * p.ks.y;
    p.kb = mk(0.04f * (1.0f - metal) + p.kd.x * metal, 0.04f * (1.0f - metal) + p.kd.y * metal, 0.04f * (1.0f - metal) + p.kd.z * metal);
    // lobe choice: diffuse albedo against the Fresnel-weighted specular colour at the view angle
    const float wd = (1.0f - metal) * luminance(p.kd);
    float ws = 0.0f;
    {
        V3 W = unit0(p.nrm), U, V;
        onb(W, U, V);
        const float c = unit0(mk(dot(p.wo, U), dot(p.wo, V), dot(p.wo, W))).z;
        if (c > 0.0f) {
            float s = 1.0f - fminf(fmaxf(c, SPEC_EPS), SPEC_ONE);
            s = powf(s, 5.0f);
            ws = luminance(mk(p.kb.x * (1.0f - s) + s, p.kb.y * (1.0f - s) + s, p.kb.z * (1.0f - s) + s));
        }
    }
    const float pD = (wd + ws) > 0.0f ? wd / (wd + ws) : 1.0f, pS = 1.0f - pD;

    unsigned s0 = a.seed, s1 = (unsigned)i;
    unsigned state = rand_pcg(s0) ^ rand_pcg(s1);
    const int* perm_l = a.perms + (size_t)(rand_pcg(state) % (unsigned)a.R) * (a.n * a.n);
    const int* perm_b = a.perms + (size_t)(rand_pcg(state) % (unsigned)a.R) * (a.n * a.n);
    const float strata = 1.0f / (float)a.n, frac = 1.0f / (float)(a.n * a.n);
    for (int k = 0; k < a.n * a.n; ++k) {
        float pdf_l, pdf_b;
        float sx = ((float)(perm_l[k] % a.n) + uniform_pcg(state)) * strata;
        float sy = ((float)(perm_l[k] / a.n) + uniform_pcg(state)) * strata;
        V3 wi = light_sample(a, sx, sy, pdf_l);
        pdf_b = bsdf_pdf(pD, pS, p.nrm, p.wo, wi, alpha);
        shade_sample<BWD>(a, p, wi, pdf_l + pdf_b, frac);

        sx = ((float)(perm_b[k] % a.n) + uniform_pcg(state)) * strata;
        sy = ((float)(perm_b[k] / a.n) + uniform_pcg(state)) * strata;
        float sz = uniform_pcg(state);
        bool lobe;
        wi = bsdf_sample(pD, pS, p.nrm, p.wo, mk(sx, sy, sz), alpha, pdf_b, lobe);
        pdf_l = light_pdf(a, wi);
        shade_sample<BWD>(a, p, wi, pdf_l + pdf_b, frac);
    }
    if (!BWD) {
        st3(a.diff + 3 * i, p.acc_diff);
        st3(a.spec + 3 * i, p.acc_spec);
    } else {
        st3(a.d_nrm + 3 * i, p.d_nrm);
        if (a.d_kd) st3(a.d_kd + 3 * i, p.d_kd);
        if (a.d_ks) st3(a.d_ks + 3 * i, p.d_ks);
        if (a.d_pos) st3(a.d_pos + 3 * i, fnormalize_bwd(wor, p.d_wo) * -1.0f);        // wo = normalize(view_pos - pos)
    }
}

int env_args(EnvArgs& a, const float* nodes, const float* tri9, int64_t F, const float* const* gb, const float* light, int LH, int LW, const float* pdf,
             const float* rows, const float* cols, int PH, int PW, const int* perms, int R, int64_t npix, int mode, int n, unsigned seed,
             float shadow_scale) {
    if (F < 0 || (F > 0 && (!nodes || !tri9)) || npix < 0 || mode < 0 || mode > 2 || n < 1 || n > 1024 || R < 1 || LH < 1 || LW < 1 || PH < 1 || PW < 1)
        return D3H_ERR_ARG;
    if (!gb || !light || !pdf || !rows || !cols || !perms) return D3H_ERR_ARG;
    for (int k = 0; k < 7; ++k)
        if (!gb[k] && npix > 0) return D3H_ERR_ARG;
    a.nodes = (const float4*)nodes; a.tri9 = tri9; a.F = (int)F;
    a.mask = gb[0]; a.ro = gb[1]; a.pos = gb[2]; a.nrm = gb[3]; a.view = gb[4]; a.kd = gb[5]; a.ks = gb[6];
    a.light = light; a.LH = LH; a.LW = LW;
    a.pdf = pdf; a.rows = rows; a.cols = cols; a.PH = PH; a.PW = PW;
    a.perms = perms; a.R = R;
    a.npix = (size_t)npix;
    a.mode = mode; a.n = n; a.seed = seed; a.shadow_scale = shadow_scale;
    a.diff = a.spec = nullptr;
    a.g_diff = a.g_spec = nullptr;
    a.d_pos = a.d_nrm = a.d_kd = a.d_ks = a.d_light = nullptr;
    return D3H_OK;
}

}  // namespace

// Shade npix = B H W pixels under the environment light.  nodes, tri9, F: the BVH of d3h_bvh_build (F = 0: nothing occludes).  gbuffer: HOST array of
// the 7 per-pixel inputs {mask [npix], ro, gb_pos, gb_normal, gb_view_pos, gb_kd, gb_ks [npix][3]}.  light [LH][LW][3]: the lat-long map, looked up
// by nearest texel.  pdf [PH][PW], rows [PH], cols [PH][PW]: texel probabilities and their row / per-row column CDFs.  perms [R][n^2] (int32):
// permutations of 0 .. n^2-1 that decorrelate the strata of the light and BSDF samples.  mode: 0 pbr, 1 diffuse, 2 white (Lambert only).  n: strata
// per axis.  diff, spec [npix][3] are overwritten (zeros where mask <= 0).
extern "C" int d3h_env_shade_fwd(const float* nodes, const float* tri9, int64_t F, const float* const* gbuffer, const float* light, int LH, int LW,
                                 const float* pdf, const float* rows, const float* cols, int PH, int PW, const int* perms, int R, int64_t npix, int mode,
                                 int n, unsigned seed, float shadow_scale, float* diff, float* spec, void* stream) {
    EnvArgs a;
    if (env_args(a, nodes, tri9, F, gbuffer, light, LH, LW, pdf, rows, cols, PH, PW, perms, R, npix, mode, n, seed, shadow_scale) != D3H_OK) return D3H_ERR_ARG;
    if (npix == 0) return D3H_OK;
    if (!diff || !spec) return D3H_ERR_ARG;
    a.diff = diff; a.spec = spec;
    hipLaunchKernelGGL(env_shade_kernel<false>, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    D3H_LAUNCH_CHECK();
    return D3H_OK;
}
// Gradients of d3h_env_shade_fwd from g_diff, g_spec [npix][3], re-sampled with `seed` and recomputed from the inputs.  d_nrm [npix][3] is
// overwritten; d_pos, d_kd, d_ks [npix][3] are overwritten, or skipped where NULL (they are zero in modes 1 and 2); d_light [LH][LW][3] is
// ACCUMULATED (float atomics: the last bits depend on their order).  Sample directions, pdfs and visibility carry no gradient.
extern "C" int d3h_env_shade_bwd(const float* nodes, const float* tri9, int64_t F, const float* const* gbuffer, const float* light, int LH, int LW,
                                 const float* pdf, const float* rows, const float* cols, int PH, int PW, const int* perms, int R, int64_t npix, int mode,
                                 int n, unsigned seed, float shadow_scale, const float* g_diff, const float* g_spec, float* d_pos, float* d_nrm,
                                 float* d_kd, float* d_ks, float* d_light, void* stream) {
    EnvArgs a;
    if (env_args(a, nodes, tri9, F, gbuffer, light, LH, LW, pdf, rows, cols, PH, PW, perms, R, npix, mode, n, seed, shadow_scale) != D3H_OK) return D3H_ERR_ARG;
    if (npix == 0) return D3H_OK;
    if (!g_diff || !g_spec || !d_nrm || !d_light) return D3H_ERR_ARG;
    a.g_diff = g_diff; a.g_spec = g_spec;
    a.d_pos = d_pos; a.d_nrm = d_nrm; a.d_kd = d_kd; a.d_ks = d_ks; a.d_light = d_light;
    hipLaunchKernelGGL(env_shade_kernel<true>, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    D3H_LAUNCH_CHECK();
    return D3H_OK;
}
