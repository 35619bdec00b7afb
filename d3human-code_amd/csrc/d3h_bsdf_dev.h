// d3h_bsdf_dev.h -- the per-pixel BSDF device functions (f = forward, b = backward with accumulated gradients) shared by bsdf.hip (the
// render.renderutils entry points) and envshade.hip (the ray-traced environment shading of render.optixutils).  The maths is that of the python
// twins, render/renderutils/bsdf.py: cosines clamped to [1e-4, 1 - 1e-4], alpha clamped to [min_roughness^2, 1], front-facing selects.
#pragma once
#include "d3h_vec.h"

namespace {

constexpr float SPEC_EPS = 1e-4f, SPEC_ONE = 0.9999f;      // bsdf.py:94 specular_epsilon and 1 - specular_epsilon
constexpr float PI_F = 3.14159265358979323846f;

__device__ __forceinline__ float clamp_cos(float c, bool& inside) {
    inside = c > SPEC_EPS && c < SPEC_ONE;
    return fminf(fmaxf(c, SPEC_EPS), SPEC_ONE);
}

// ---- the scalar pieces: f(...) and b(..., g, accumulated gradients) -------------------------------------------------------------
// f0 + (f90 - f0) (1 - cos)^5
__device__ __forceinline__ float shlick_f(float f0, float f90, float c) {
    bool in;
    float s = 1.0f - clamp_cos(c, in), s2 = s * s;
    return f0 + (f90 - f0) * (s2 * s2 * s);
}
__device__ __forceinline__ void shlick_b(float f0, float f90, float c, float g, float& d_f0, float& d_f90, float& d_c) {
    bool in;
    float s = 1.0f - clamp_cos(c, in), s2 = s * s, s4 = s2 * s2, s5 = s4 * s;
    d_f0 += g * (1.0f - s5);
    d_f90 += g * s5;
    if (in) d_c += g * (f90 - f0) * (-5.0f * s4);
}
// alpha^2 / (pi d^2), d = (cos alpha^2 - cos) cos + 1
__device__ __forceinline__ float ndf_f(float a2, float c) {
    bool in;
    float cc = clamp_cos(c, in);
    float d = (cc * a2 - cc) * cc + 1.0f;
    return a2 / (d * d * PI_F);
}
__device__ __forceinline__ void ndf_b(float a2, float c, float g, float& d_a2, float& d_c) {
    bool in;
    float cc = clamp_cos(c, in);
    float d = (cc * a2 - cc) * cc + 1.0f;
    float inv = 1.0f / (d * d * PI_F);
    float g_d = g * (-2.0f * a2 * inv / d);
    d_a2 += g * inv + g_d * (cc * cc);
    if (in) d_c += g_d * (2.0f * cc * (a2 - 1.0f));
}
// (sqrt(1 + alpha^2 tan^2) - 1) / 2
__device__ __forceinline__ float lambda_f(float a2, float c) {
    bool in;
    float cc = clamp_cos(c, in), c2 = cc * cc;
    float t2 = (1.0f - c2) / c2;
    return 0.5f * (sqrtf(1.0f + a2 * t2) - 1.0f);
}
__device__ __forceinline__ void lambda_b(float a2, float c, float g, float& d_a2, float& d_c) {
    bool in;
    float cc = clamp_cos(c, in), c2 = cc * cc;
    float t2 = (1.0f - c2) / c2;
    float gr = g * 0.25f / sqrtf(1.0f + a2 * t2);           // g d(out)/d(1 + a2 t2)
    d_a2 += gr * t2;
    if (in) d_c += gr * a2 * (-2.0f / (c2 * cc));           // t2 = 1 / cos^2 - 1
}
// 1 / (1 + lambda(cos_i) + lambda(cos_o))
__device__ __forceinline__ float smith_f(float a2, float ci, float co) { return 1.0f / (1.0f + lambda_f(a2, ci) + lambda_f(a2, co)); }
__device__ __forceinline__ void smith_b(float a2, float ci, float co, float g, float& d_a2, float& d_ci, float& d_co) {
    float o = smith_f(a2, ci, co);
    float gl = -g * o * o;
    lambda_b(a2, ci, gl, d_a2, d_ci);
    lambda_b(a2, co, gl, d_a2, d_co);
}

// ---- the lobes ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float lambert_f(V3 n, V3 wi) { return fmaxf(dot(n, wi), 0.0f) / PI_F; }
__device__ __forceinline__ void lambert_b(V3 n, V3 wi, float g, V3& d_n, V3& d_wi) {
    if (dot(n, wi) > 0.0f) {
        float s = g / PI_F;
        d_n = d_n + wi * s;
        d_wi = d_wi + n * s;
    }
}

constexpr float FROST_K = 0.51f / 1.51f;
__device__ __forceinline__ float frostbite_f(V3 n, V3 wi, V3 wo, float lr) {
    float wiN = dot(wi, n), woN = dot(wo, n);
    V3 h = fnormalize(wo + wi);
    float wiH = dot(wi, h);
    float f90 = 0.5f * lr + 2.0f * wiH * wiH * lr;
    float res = shlick_f(1.0f, f90, wiN) * shlick_f(1.0f, f90, woN) * (1.0f - FROST_K * lr);
    return (wiN > 0.0f && woN > 0.0f) ? res : 0.0f;
}
__device__ __forceinline__ void frostbite_b(V3 n, V3 wi, V3 wo, float lr, float g, V3& d_n, V3& d_wi, V3& d_wo, float& d_lr) {
    float wiN = dot(wi, n), woN = dot(wo, n);
    if (!(wiN > 0.0f && woN > 0.0f)) return;
    V3 hr = wo + wi, h = fnormalize(hr);
    float wiH = dot(wi, h);
    float f90 = 0.5f * lr + 2.0f * wiH * wiH * lr, ef = 1.0f - FROST_K * lr;
    float si = shlick_f(1.0f, f90, wiN), so = shlick_f(1.0f, f90, woN);
    float g_f0 = 0.f, g_f90 = 0.f, g_wiN = 0.f, g_woN = 0.f;
    shlick_b(1.0f, f90, wiN, g * so * ef, g_f0, g_f90, g_wiN);
    shlick_b(1.0f, f90, woN, g * si * ef, g_f0, g_f90, g_woN);
    d_lr += g * si * so * (-FROST_K) + g_f90 * (0.5f + 2.0f * wiH * wiH);
    float g_wiH = g_f90 * 4.0f * wiH * lr;
    V3 g_hr = fnormalize_bwd(hr, wi * g_wiH);
    d_wi = d_wi + h * g_wiH + n * g_wiN + g_hr;
    d_wo = d_wo + n * g_woN + g_hr;
    d_n = d_n + wi * g_wiN + wo * g_woN;
}

__device__ __forceinline__ V3 specular_f(V3 col, V3 n, V3 wo, V3 wi, float alpha, float alpha_min) {
    float a = fminf(fmaxf(alpha, alpha_min), 1.0f), a2 = a * a;
    V3 h = fnormalize(wo + wi);
    float woN = dot(wo, n), wiN = dot(wi, n), woH = dot(wo, h), nH = dot(n, h);
    float k = ndf_f(a2, nH) * smith_f(a2, woN, wiN) * 0.25f / fmaxf(woN, SPEC_EPS);
    if (!(woN > SPEC_EPS && wiN > SPEC_EPS)) return mk(0.f, 0.f, 0.f);
    return mk(shlick_f(col.x, 1.0f, woH) * k, shlick_f(col.y, 1.0f, woH) * k, shlick_f(col.z, 1.0f, woH) * k);
}
__device__ __forceinline__ void specular_b(V3 col, V3 n, V3 wo, V3 wi, float alpha, float alpha_min, V3 g, V3& d_col, V3& d_n, V3& d_wo, V3& d_wi,
                                           float& d_alpha) {
    float woN = dot(wo, n), wiN = dot(wi, n);
    if (!(woN > SPEC_EPS && wiN > SPEC_EPS)) return;
    float a = fminf(fmaxf(alpha, alpha_min), 1.0f), a2 = a * a;
    V3 hr = wo + wi, h = fnormalize(hr);
    float woH = dot(wo, h), nH = dot(n, h);
    float D = ndf_f(a2, nH), G = smith_f(a2, woN, wiN);
    float q = 0.25f / woN;                               // front facing: clamp(woN, min = eps) = woN, and it passes its gradient
    V3 F = mk(shlick_f(col.x, 1.0f, woH), shlick_f(col.y, 1.0f, woH), shlick_f(col.z, 1.0f, woH));
    float k = D * G * q, s = dot(g, F);
    float g_a2 = 0.f, g_nH = 0.f, g_woN = -s * D * G * q / woN, g_wiN = 0.f, g_woH = 0.f, g_f90 = 0.f;
    ndf_b(a2, nH, s * G * q, g_a2, g_nH);
    smith_b(a2, woN, wiN, s * D * q, g_a2, g_woN, g_wiN);
    V3 gc = mk(0.f, 0.f, 0.f);
    shlick_b(col.x, 1.0f, woH, g.x * k, gc.x, g_f90, g_woH);
    shlick_b(col.y, 1.0f, woH, g.y * k, gc.y, g_f90, g_woH);
    shlick_b(col.z, 1.0f, woH, g.z * k, gc.z, g_f90, g_woH);
    d_col = d_col + gc;
    if (alpha > alpha_min && alpha < 1.0f) d_alpha += g_a2 * 2.0f * a;
    V3 g_hr = fnormalize_bwd(hr, wo * g_woH + n * g_nH);
    d_wo = d_wo + h * g_woH + n * g_woN + g_hr;
    d_wi = d_wi + n * g_wiN + g_hr;
    d_n = d_n + wo * g_woN + wi * g_wiN + h * g_nH;
}

}  // namespace
