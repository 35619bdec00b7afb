// envlight.hip -- the sampling tables of the lat-long environment light: pdf, column CDFs, row CDF.
//
// Replaces (reference file:line): render/light.py:46-59 (EnvironmentLight.update_pdf: max over channels, sin(theta) weight, two cumsums, two
// normalisations -- about ten torch launches per training iteration).  Two launches here, no atomics, no host synchronisation.
//
// The sampler (csrc/envshade.hip) searches these tables, so three properties hold EXACTLY, not to rounding (light >= 0):
//   * every table is non-decreasing;  * cols[y][W-1] == 1 on every row with a positive total;  * rows[H-1] == 1.
// A parallel scan in float does not give the first one by itself (two prefix sums formed along different trees can come out in the wrong order by
// an ulp), so every prefix sum here has the form fl(offset_t + run), where thread t owns a CONTIGUOUS segment, `run` is its sequential running sum
// and the offsets are the sequential sum of the segment totals: within a segment fl(offset + run) is monotone in run because rounding is monotone,
// and the last entry of segment t, fl(offset_t + total_t), IS offset_{t+1}.  The normalisations divide by the table's own last entry: x / x == 1, and
// a correctly rounded division by a positive constant is monotone.
#include "d3h_common.h"

namespace {

constexpr int EL_T = 256;
constexpr float EL_PI = 3.14159265358979323846f;

__device__ __forceinline__ float el_texel(const float* __restrict__ base, size_t i, float s) {
    return fmaxf(fmaxf(base[3 * i], base[3 * i + 1]), base[3 * i + 2]) * s;
}

// the sequential exclusive sum of the 256 segment totals, by thread 0: off[0 .. 256], off[256] the total.  Every thread calls it.
__device__ __forceinline__ void el_offsets(float part, float* off, float* tmp) {
    tmp[threadIdx.x] = part;
    __syncthreads();
    if (threadIdx.x == 0) {
        float o = 0.f;
        for (int t = 0; t < EL_T; ++t) { off[t] = o; o += tmp[t]; }
        off[EL_T] = o;
    }
    __syncthreads();
}

// one workgroup per row: p = max(rgb) sin(pi (y + 0.5) / H) -> pdf (not yet normalised), its normalised inclusive sum -> cols, its total -> rowtot
__global__ __launch_bounds__(EL_T) void envlight_row_kernel(const float* __restrict__ base, int H, int W, float* __restrict__ pdf, float* __restrict__ cols,
                                                            float* __restrict__ rowtot) {
    __shared__ float off[EL_T + 1], tmp[EL_T];
    const int y = blockIdx.x;
    const float s = sinf(((float)y + 0.5f) / (float)H * EL_PI);
    const int seg = (W + EL_T - 1) / EL_T;
    const int x0 = min((int)threadIdx.x * seg, W), x1 = min(x0 + seg, W);
    const size_t row = (size_t)y * W;
    float run = 0.f;
    for (int x = x0; x < x1; ++x) run += el_texel(base, row + x, s);
    el_offsets(run, off, tmp);
    const float tot = off[EL_T], den = tot > 0.f ? tot : 1.0f, o = off[threadIdx.x];
    run = 0.f;
    for (int x = x0; x < x1; ++x) {
        const float p = el_texel(base, row + x, s);
        run += p;
        pdf[row + x] = p;
        cols[row + x] = (o + run) / den;
    }
    if (threadIdx.x == 0) rowtot[y] = tot;
}

// every workgroup forms the SAME sum of the row totals (same order: same bits) and normalises its 1024 texels of pdf; workgroup 0 also writes rows
__global__ __launch_bounds__(EL_T) void envlight_norm_kernel(const float* __restrict__ rowtot, int H, int64_t n, float* __restrict__ pdf, float* __restrict__ rows) {
    __shared__ float off[EL_T + 1], tmp[EL_T];
    const int seg = (H + EL_T - 1) / EL_T;
    const int y0 = min((int)threadIdx.x * seg, H), y1 = min(y0 + seg, H);
    float run = 0.f;
    for (int y = y0; y < y1; ++y) run += rowtot[y];
    el_offsets(run, off, tmp);
    const float tot = off[EL_T];
    const int64_t i0 = (int64_t)blockIdx.x * (4 * EL_T);
    for (int k = 0; k < 4; ++k) {
        const int64_t i = i0 + k * EL_T + threadIdx.x;
        if (i < n) pdf[i] = pdf[i] / tot;
    }
    if (blockIdx.x == 0) {
        const float den = tot > 0.f ? tot : 1.0f, o = off[threadIdx.x];
        run = 0.f;
        for (int y = y0; y < y1; ++y) {
            run += rowtot[y];
            rows[y] = (o + run) / den;
        }
    }
}

}  // namespace

// Sampling tables of a lat-long environment map base [H][W][3] (>= 0): pdf [H][W] := max(rgb) sin(pi (y + 0.5) / H) / (sum of that over the map);
// cols [H][W] := inclusive sum of a row / the row's total (/ 1 where the total is 0: such a row is all 0); rows [H] := inclusive sum of the row
// totals / its last entry.  All overwritten; rowtot [H] is scratch.  Tables are non-decreasing, cols[y][W-1] == 1 on rows with a positive total and
// rows[H-1] == 1, exactly.  Two launches, no atomics: identical bits from run to run.  A map whose pdf sums to 0 is 0 / 0 (unspecified).
extern "C" int d3h_envlight_tables(const float* base, int H, int W, float* pdf, float* rows, float* cols, float* rowtot, void* stream) {
    if (H < 1 || W < 1 || !base || !pdf || !rows || !cols || !rowtot) return D3H_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    const int64_t n = (int64_t)H * W;
    if ((n + 4 * EL_T - 1) / (4 * EL_T) > 0x7fffffff) return D3H_ERR_ARG;
    hipLaunchKernelGGL(envlight_row_kernel, dim3((unsigned)H), dim3(EL_T), 0, s, base, H, W, pdf, cols, rowtot);
    D3H_LAUNCH_CHECK();
    hipLaunchKernelGGL(envlight_norm_kernel, dim3((unsigned)((n + 4 * EL_T - 1) / (4 * EL_T))), dim3(EL_T), 0, s, (const float*)rowtot, H, n, pdf, rows);
    D3H_LAUNCH_CHECK();
    return D3H_OK;
}
