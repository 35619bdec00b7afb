// cubemap.hip -- the two cube-map filters of render.renderutils on gfx950: the cosine-lobe (diffuse) and the GGX-lobe (specular, split-sum)
// pre-filter of an environment map [6][N][N][3], forward and backward.
//
// Replaces (reference file:line): render/renderutils/c_src/cubemap.cu:110-169 (diffuse), :246-350 (specular) and the host recipe of
// render/renderutils/ops.py:394-461.  Semantics kept: cube_to_dir's side table (the one of render/util.py), pixel_area exactly as it is (its sum
// over the cube is not 4 pi), the diffuse weight clamp(dot, 0, 0.999) area / 3.141592, the specular cone test dot >= costheta_cutoff with
// weight max(dot, 0) D_ggx(roughness^4, max(dot(d_p, h), 0)) area / 4, result sum(w c) / sum(w).
//
// Shape of the computation: a pair sweep, 6 N^2 outputs x 6 N^2 inputs.  The per-texel direction and area depend on N alone and come from a
// table {d.xyz, area} built once per N (d3h_cubemap_table), so no atan / rsqrt is redone per pair.  Work is cut into 16 x 16 patches of a
// face: one workgroup owns the outputs of one patch (one thread per texel) and walks over the input patches, staging each through LDS (table
// entry + 3 values per texel; all lanes read the same LDS address: a broadcast).  Every patch has a bounding cone {axis, half angle} (host,
// d3h/cubemap.py); an input patch whose cone is further from the output patch's than the filter reaches -- the cutoff angle of the specular
// lobe, 90 degrees for the diffuse one -- is skipped by the whole workgroup.  That is the job of the reference's per-texel bounding rectangles,
// done per patch pair: conservative, so the result is that of the sum over all pairs; inside a kept patch every pair is tested.
// The backward is a GATHER with the same tables (the cone test is symmetric in the two texels): grad_cubemap[q] = area(q) sum_p (...) g[p]
// -- no atomics, bit-reproducible; the reference scatters with float atomics.
#include "d3h_vec.h"

namespace {

constexpr int CM_TILE = 256;
constexpr float CM_PI = 3.14159265358979323846f;
enum { CM_DIFFUSE_FWD = 0, CM_DIFFUSE_BWD = 1, CM_SPECULAR_FWD = 2, CM_SPECULAR_BWD = 3 };

// texel (x, y) of face `side` -> unit direction (faces +x, -x, +y, -y, +z, -z)
__device__ __forceinline__ V3 cube_to_dir(int x, int y, int side, int N) {
    float fx = 2.0f * (((float)x + 0.5f) / (float)N) - 1.0f;
    float fy = 2.0f * (((float)y + 0.5f) / (float)N) - 1.0f;
    V3 v;
    switch (side) {
        case 0: v = mk(1.0f, -fy, -fx); break;
        case 1: v = mk(-1.0f, -fy, fx); break;
        case 2: v = mk(fx, 1.0f, fy); break;
        case 3: v = mk(fx, -1.0f, -fy); break;
        case 4: v = mk(fx, -fy, 1.0f); break;
        default: v = mk(-fx, -fy, -1.0f); break;
    }
    return v * (1.0f / sqrtf(dot(v, v)));
}
// the texel weight of the reference: product of two atan differences with H = N / 2 (integer), 1 for N = 1
__device__ __forceinline__ float pixel_area(int x, int y, int N) {
    if (N <= 1) return 1.0f;
    int H = N / 2;
    x = abs(x - H); y = abs(y - H);
    float dx = atanf((float)(x + 1) / (float)H) - atanf((float)x / (float)H);
    float dy = atanf((float)(y + 1) / (float)H) - atanf((float)y / (float)H);
    return dx * dy;
}

__global__ __launch_bounds__(256) void cubemap_table_kernel(int N, float4* __restrict__ table) {
    int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= 6 * N * N) return;
    int side = t / (N * N), y = (t / N) % N, x = t % N;
    V3 d = cube_to_dir(x, y, side, N);
    table[t] = make_float4(d.x, d.y, d.z, pixel_area(x, y, N));
}

__device__ __forceinline__ float ndf_ggx01(float a2, float c) {
    c = fminf(fmaxf(c, 0.0f), 1.0f);
    float d = (c * a2 - c) * c + 1.0f;
    return a2 / (d * d * CM_PI);
}

// sum += v with the running compensation c (Kahan); relies on the build's strict float semantics (no fast-math, no contraction)
__device__ __forceinline__ void kahan_add(float& sum, float& c, float v) {
    float y = v - c, t = sum + y;
    c = (t - sum) - y;
    sum = t;
}

constexpr int CM_P = 16;            // patch edge: CM_P^2 = CM_TILE staging slots
struct CmPatch { int side, x0, y0, w, h; };
// patch t of the ppf x ppf patches per face (row-major inside a face, faces in order); w, h: its extent inside the N x N face
__device__ __forceinline__ CmPatch cm_patch(int t, int N, int ppf) {
    CmPatch p;
    p.side = t / (ppf * ppf);
    int r = t % (ppf * ppf);
    p.y0 = (r / ppf) * CM_P; p.x0 = (r % ppf) * CM_P;
    p.w = N - p.x0 < CM_P ? N - p.x0 : CM_P;
    p.h = N - p.y0 < CM_P ? N - p.y0 : CM_P;
    return p;
}

// one (output texel i, input texel j) pair: ta += weight v, tw += weight (the weights: see the kernel)
template <int MODE>
__device__ __forceinline__ void cm_pair(V3 di, float4 tj, const float* v, float a2, float cut, V3& ta, float& tw) {
    constexpr bool FWD = MODE == CM_DIFFUSE_FWD || MODE == CM_SPECULAR_FWD;
    constexpr bool SPEC = MODE == CM_SPECULAR_FWD || MODE == CM_SPECULAR_BWD;
    const V3 dj = mk(tj.x, tj.y, tj.z);
    const float dt = dot(di, dj);
    float w;
    if (SPEC) {
        if (!(dt >= cut)) return;
        V3 hs = di + dj;
        V3 h = hs * (1.0f / sqrtf(fmaxf(dot(hs, hs), 1e-20f)));
        w = fmaxf(dt, 0.0f) * ndf_ggx01(a2, fmaxf(dot(FWD ? di : dj, h), 0.0f));
    } else {
        w = fminf(fmaxf(dt, 0.0f), 0.999f);
    }
    if (FWD) w *= tj.w;
    ta = ta + mk(v[0], v[1], v[2]) * w;
    tw += w;
}

// out[i] = sum_j weight(i, j) val[j] over the n = 6 N^2 texels.
//   diffuse  fwd: weight = clamp(d_i . d_j, 0, 0.999) area_j / 3.141592;          val = cubemap
//   diffuse  bwd: weight = clamp(d_i . d_j, 0, 0.999) area_i / 3.141592;          val = g_out
//   specular fwd: weight = [d_i . d_j >= cut] max(d_i . d_j, 0) D(d_i . h) area_j / 4;  val = cubemap;  out = sum / sum of weights -> wsum[i]
//   specular bwd: weight = [d_i . d_j >= cut] max(d_i . d_j, 0) D(d_j . h) area_i / 4;  val = g_out[j] / wsum[j]
// cones[t] = {axis, half angle} of patch t; reach: the largest angle between two texels with a non-zero weight (plus a rounding margin)
template <int MODE>
__global__ __launch_bounds__(256) void cubemap_filter_kernel(const float4* __restrict__ table, const float4* __restrict__ cones, const float* __restrict__ val,
                                                             const float* __restrict__ wsum_in, int N, int ppf, float a2, float cut, float reach,
                                                             float* __restrict__ out, float* __restrict__ wsum_out) {
    __shared__ float4 s_t[CM_TILE];
    __shared__ float s_v[CM_TILE * 3];
    constexpr bool FWD = MODE == CM_DIFFUSE_FWD || MODE == CM_SPECULAR_FWD;
    constexpr bool SPEC = MODE == CM_SPECULAR_FWD || MODE == CM_SPECULAR_BWD;
    const int tid = threadIdx.x, lx = tid & (CM_P - 1), ly = tid / CM_P;
    const int npatch = 6 * ppf * ppf;
    const CmPatch me = cm_patch(blockIdx.x, N, ppf);
    const bool live = lx < me.w && ly < me.h;
    const int i = live ? (me.side * N + me.y0 + ly) * N + me.x0 + lx : 0;
    const float4 ti = live ? table[i] : make_float4(0.f, 0.f, 1.f, 0.f);
    const V3 di = mk(ti.x, ti.y, ti.z);
    const float4 cme = cones[blockIdx.x];
    // Summation: a patch's terms are added in order into patch partials; the partials go into the running totals with a compensated
    // (Kahan) add, so the rounding error does not grow with the number of patches (one plain chain over 6 N^2 same-sign terms loses ~sqrt(6 N^2)
    // ulp: 1.7e-6 at N = 16, beyond what a float32 pairwise sum of the same terms is off by)
    V3 acc = mk(0.f, 0.f, 0.f), acc_c = mk(0.f, 0.f, 0.f);
    float wsum = 0.f, wsum_c = 0.f;
    for (int t = 0; t < npatch; ++t) {
        const float4 ct = cones[t];
        const float span = cme.w + ct.w + reach;             // workgroup-uniform: no texel of patch t is within `reach` of a texel of mine
        if (span < 3.1f && cme.x * ct.x + cme.y * ct.y + cme.z * ct.z < cosf(span)) continue;
        const CmPatch p = cm_patch(t, N, ppf);
        if (lx < p.w && ly < p.h) {                         // stage the patch: slot tid = texel (x0 + lx, y0 + ly)
            const int j = (p.side * N + p.y0 + ly) * N + p.x0 + lx;
            s_t[tid] = table[j];
            V3 v = ld3(val + 3 * (size_t)j);
            if (MODE == CM_SPECULAR_BWD) v = v * (1.0f / wsum_in[j]);
            s_v[3 * tid] = v.x; s_v[3 * tid + 1] = v.y; s_v[3 * tid + 2] = v.z;
        }
        __syncthreads();
        if (live) {
            V3 ta = mk(0.f, 0.f, 0.f);
            float tw = 0.f;
            if (p.w == CM_P && p.h == CM_P) {               // a full patch: a fixed trip count the compiler unrolls
#pragma unroll 8
                for (int k = 0; k < CM_TILE; ++k) cm_pair<MODE>(di, s_t[k], s_v + 3 * k, a2, cut, ta, tw);
            } else {
                for (int ky = 0; ky < p.h; ++ky)
                    for (int kx = 0; kx < p.w; ++kx) cm_pair<MODE>(di, s_t[ky * CM_P + kx], s_v + 3 * (ky * CM_P + kx), a2, cut, ta, tw);
            }
            kahan_add(acc.x, acc_c.x, ta.x); kahan_add(acc.y, acc_c.y, ta.y); kahan_add(acc.z, acc_c.z, ta.z);
            kahan_add(wsum, wsum_c, tw);
        }
        __syncthreads();
    }
    if (!live) return;
    const float norm = SPEC ? 0.25f : 1.0f / 3.141592f;
    if (MODE == CM_SPECULAR_FWD) {
        wsum_out[i] = wsum * norm;
        acc = acc * (1.0f / wsum);
    } else {
        acc = acc * (FWD ? norm : norm * ti.w);
    }
    st3(out + 3 * (size_t)i, acc);
}

inline bool cm_bad_n(int N) { return N < 1 || N > 8192; }
inline int cm_ppf(int N) { return (N + CM_P - 1) / CM_P; }
constexpr float CM_MARGIN = 2e-3f;          // radians added to the filter's reach: rounding of the cones, of acosf / cosf and of the dot products

template <int MODE>
int cm_launch(const float* table, const float* cones, const float* val, const float* wsum_in, int N, float roughness, float cut, float reach, float* out,
              float* wsum_out, void* stream) {
    if (cm_bad_n(N) || !table || !cones || !val || !out) return D3H_ERR_ARG;
    const int ppf = cm_ppf(N);
    const float alpha = roughness * roughness;
    hipLaunchKernelGGL(cubemap_filter_kernel<MODE>, dim3(6 * ppf * ppf), dim3(CM_TILE), 0, (hipStream_t)stream, (const float4*)table, (const float4*)cones, val,
                       wsum_in, N, ppf, alpha * alpha, cut, reach + CM_MARGIN, out, wsum_out);
    D3H_LAUNCH_CHECK();
    return D3H_OK;
}
inline float cm_cone_angle(float costheta_cutoff) { return acosf(fminf(fmaxf(costheta_cutoff, -1.0f), 1.0f)); }

}  // namespace

// table [6 N^2][4] = {unit direction xyz, pixel_area} of every texel of an N x N cube map, texel order [side][y][x]
extern "C" int d3h_cubemap_table(int N, float* table, void* stream) {
    if (cm_bad_n(N) || !table) return D3H_ERR_ARG;
    const int n = 6 * N * N;
    hipLaunchKernelGGL(cubemap_table_kernel, dim3(d3h_cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, N, (float4*)table);
    D3H_LAUNCH_CHECK();
    return D3H_OK;
}
// diffuse_cubemap.  backward = 0: val = cubemap [6][N][N][3] -> out = the filtered map; backward = 1: val = the gradient of the filtered map -> out
// = the gradient of the cubemap (a gather, no atomics).  out is overwritten.  table: d3h_cubemap_table(N); cones [6 ceil(N / 16)^2][4] = {unit axis,
// half angle in radians} of a cone that holds every texel direction of each 16 x 16 patch (patches row-major inside a face, faces in order).
extern "C" int d3h_cubemap_diffuse(const float* table, const float* cones, const float* val, int N, int backward, float* out, void* stream) {
    const float reach = 1.57079633f;        // the clamp of the cosine at 0: nothing beyond 90 degrees contributes
    return backward ? cm_launch<CM_DIFFUSE_BWD>(table, cones, val, nullptr, N, 0.f, 0.f, reach, out, nullptr, stream)
                    : cm_launch<CM_DIFFUSE_FWD>(table, cones, val, nullptr, N, 0.f, 0.f, reach, out, nullptr, stream);
}
// specular_cubemap, forward: out [6][N][N][3] = sum(w c) / sum(w) over the texels inside the cone dot >= costheta_cutoff; wsum [6 N^2] = sum(w)
// (kept by the caller for the backward).  Both overwritten.  table, cones: as for d3h_cubemap_diffuse.
extern "C" int d3h_cubemap_specular_fwd(const float* table, const float* cones, const float* cubemap, int N, float roughness, float costheta_cutoff, float* out,
                                        float* wsum, void* stream) {
    if (!wsum) return D3H_ERR_ARG;
    return cm_launch<CM_SPECULAR_FWD>(table, cones, cubemap, nullptr, N, roughness, costheta_cutoff, cm_cone_angle(costheta_cutoff), out, wsum, stream);
}
// specular_cubemap, backward: d_cubemap [6][N][N][3] (overwritten) from g_out [6][N][N][3] and the forward's wsum; a gather, no atomics
extern "C" int d3h_cubemap_specular_bwd(const float* table, const float* cones, const float* g_out, const float* wsum, int N, float roughness,
                                        float costheta_cutoff, float* d_cubemap, void* stream) {
    if (!wsum) return D3H_ERR_ARG;
    return cm_launch<CM_SPECULAR_BWD>(table, cones, g_out, wsum, N, roughness, costheta_cutoff, cm_cone_angle(costheta_cutoff), d_cubemap, nullptr, stream);
}
