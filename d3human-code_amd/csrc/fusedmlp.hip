// fusedmlp.hip -- general fused bias-free MLP (tiny-cuda-nn "FullyFusedMLP" / "CutlassMLP"), forward and backward, for gfx950.
//
// n_in -> W -> ... -> W -> n_out with W in {16, 32, 64, 128}, 1..8 hidden layers, n_in 1..256, n_out 1..128; layer l is h <- act(h M_l^T) with
// M_l in nn.Linear layout [fan_out][fan_in], row-major float32.  tiny-cuda-nn is an un-vendored dependency of the reference (README.md:30):
// "parity unpinned", the contract is the docstring of d3h/fusedmlp.py, pinned against the float64 restatement of tests/fusedmlp_cases.py.
//
// MI355X design ("general fused MLP"):
//  - exact-f32 matrix instruction v_mfma_f32_16x16x4_f32: every dot product is an fmaf chain (the 2e-4 texture bar), and the kernel is
//    outside the co-residency rule of csrc/sdf_mlp_x3.h (no 16-bit MFMA, no register-file claim);
//  - a workgroup of 4 waves owns a tile of 64 rows, a wave 16 of them.  The wave computes Z^T = M H^T: the A operand is a 16 x 4 piece of
//    the weights (one ds_read_b128 per 4 instructions from the LDS image of the layer, rows padded by 4 floats so that the 16 rows of a
//    read fall on distinct banks), the B operand is the activation.  The D layout of the instruction (lane = row of the tile, registers =
//    4 consecutive neurons) IS a valid B operand of the next layer when that layer sums its inputs in the order 4 (l >> 4) + r inside a
//    block of 16 -- so the activations of the tile never leave the registers, forward or backward.  The same holds for the data
//    gradient dA = M^T dZ (the weights are read transposed from the same LDS image, conflict-free ds_read_b32);
//  - one "stage" = one matrix (the first in K-chunks of 128 columns) is staged in LDS at a time: at most 128 x 132 floats = 66 KB.
//    Ragged n_in / n_out are zero-padded in the LDS image and in the operand loads, never in the caller's buffers;
//    when the images of all matrices (in the backward: and the partial sums below) take at most 80 KB -- two workgroups still fit a CU --
//    they are staged once per workgroup, side by side, and the tile loop has no barrier at all: the waves run independently;
//  - activations are selected by a wave-uniform run-time switch: four instantiations per kernel (the widths);
//  - the backward stores nothing between layers but registers: it reads x, the weights and g_out, recomputes the forward of its tile, and
//    -- the derivative of every activation being a function of the post-activation value -- walks down the layers, re-running the forward
//    up to layer l for the input of matrix l (a triangular number of layer evaluations: 1 extra for 2 hidden layers, 3 for 3, 28 for 8);
//  - d_w: dM_l = dZ_l^T A_l is a sum over rows, so both operands are transposed 16 x 16 at a time through a 1 KB per-wave LDS buffer, and
//    the 16 x 16 products are added (ds_add_f32) to per-workgroup partial sums in LDS that live across the persistent tile loop and are
//    flushed ONCE per workgroup with global float atomics: the last bits of d_w depend on the order of arrival.  When the partial sums of
//    all matrices do not fit the 160 KB next to the weight image (W = 128), the grid gets one y-slice per stage and a workgroup keeps
//    the sums of its stage only (it still walks the chain down to that layer);
//  - persistent grid: min(tiles, CUs x workgroups per CU); max_cus > 0 launches exactly min(tiles, max_cus) workgroups.
//
// Bounds.  Rows: every access to x / mask / g_out / out / d_x is guarded by row < n; columns by k < n_in or c < n_out; weights and their
// gradients by o < fan_out and k < fan_in of the matrix.  LDS: the image of a stage is FO x (kc + 4) floats with FO = round_up(fan_out, 16)
// and kc a multiple of 16, every read is row < FO, column < kc; the entry point sizes the launch's LDS from the same plan.
#include "d3h_common.h"

namespace {

constexpr int FM_MAXL = 9;          // matrices
constexpr int FM_MAXS = 10;         // stages: the first matrix is at most two K-chunks
constexpr int FM_KC = 128;
constexpr int FM_PAD = 4;
constexpr int FM_TB = 16 * 17;      // per-wave transposition buffer
constexpr int FM_LDS_MAX = 160 * 1024;
constexpr int FM_LDS_RESIDENT = 80 * 1024;   // all images (and partial sums) resident while two workgroups still fit a CU
enum { FM_NONE = 0, FM_RELU = 1, FM_LEAKY = 2, FM_SIGMOID = 3, FM_TANH = 4, FM_SOFTPLUS = 5, FM_EXP = 6, FM_NACT = 7 };

struct FmPlan {
    int n_in, n_out, n_hidden, width, act, out_act;
    int n_stages, n0;               // n0: stages of matrix 0; matrix l >= 1 is stage n0 - 1 + l
    int all_groups;                 // backward: 1 = every workgroup keeps the partial sums of every stage, 0 = of stage blockIdx.y only
    int resident;                   // 1 = the images of all stages sit in LDS side by side for the whole launch, 0 = one at a time
    int sw_floats, sdw_floats;      // LDS: the weight image(s), the partial sums
    int sw_max, sw_total;           // the largest image, all images
    int st_layer[FM_MAXS], st_k0[FM_MAXS], st_kc[FM_MAXS], st_dwoff[FM_MAXS], st_swoff[FM_MAXS];
    const float* w[FM_MAXL];
    float* dw[FM_MAXL];
};

__device__ __forceinline__ float fm_act(float z, int a) {
    switch (a) {
        case FM_RELU: return fmaxf(z, 0.f);
        case FM_LEAKY: return z > 0.f ? z : 0.01f * z;
        case FM_SIGMOID: return 1.f / (1.f + expf(-z));
        case FM_TANH: return tanhf(z);
        case FM_SOFTPLUS: return fmaxf(z, 0.f) + log1pf(expf(-fabsf(z)));
        case FM_EXP: return expf(z);
        default: return z;
    }
}

// d act / d z as a function of the POST-activation value y
__device__ __forceinline__ float fm_dact(float y, int a) {
    switch (a) {
        case FM_RELU: return y > 0.f ? 1.f : 0.f;
        case FM_LEAKY: return y > 0.f ? 1.f : 0.01f;
        case FM_SIGMOID: return y * (1.f - y);
        case FM_TANH: return 1.f - y * y;
        case FM_SOFTPLUS: return -expm1f(-y);
        case FM_EXP: return y;
        default: return 1.f;
    }
}

template <int W> __device__ __forceinline__ int fm_fan_in(const FmPlan& P, int l) { return l == 0 ? P.n_in : W; }
template <int W> __device__ __forceinline__ int fm_fan_out(const FmPlan& P, int l) { return l == P.n_hidden ? P.n_out : W; }

// the LDS image of stage s: [round_up(fan_out, 16)][kc + 4], zero outside the matrix.  The caller brackets it with barriers.
template <int W> __device__ __forceinline__ void fm_stage(const FmPlan& P, int s, float* __restrict__ sw) {
    const int l = P.st_layer[s], k0 = P.st_k0[s], kc = P.st_kc[s], ld = kc + FM_PAD;
    const int fi = fm_fan_in<W>(P, l), fo = fm_fan_out<W>(P, l), FO = (fo + 15) & ~15;
    const float* __restrict__ w = P.w[l];
    for (int idx = threadIdx.x; idx < FO * kc; idx += 256) {
        const int o = idx / kc, k = idx - o * kc;
        sw[o * ld + k] = (o < fo && k0 + k < fi) ? w[(size_t)o * fi + k0 + k] : 0.f;
    }
}

// the image of stage s: resident, or staged now (every wave of the workgroup calls it: barriers)
template <int W> __device__ __forceinline__ const float* fm_weights(const FmPlan& P, int s, float* __restrict__ smem) {
    float* sw = smem + P.st_swoff[s];
    if (!P.resident) {
        __syncthreads();
        fm_stage<W>(P, s, sw);
        __syncthreads();
    }
    return sw;
}

template <int W> __device__ __forceinline__ void fm_preload(const FmPlan& P, float* __restrict__ smem) {
    if (P.resident)
        for (int s = 0; s < P.n_stages; ++s) fm_stage<W>(P, s, smem + P.st_swoff[s]);
    __syncthreads();
}

__device__ __forceinline__ f32x4 fm_zero() {
    f32x4 z = {0.f, 0.f, 0.f, 0.f};
    return z;
}

// acc += M[16 ob + i][16 t + k] (the staged image) times the activation block b (its k-th input is register r of lane group q: k = 4 q + r)
__device__ __forceinline__ f32x4 fm_mm(const float* __restrict__ sw, int ld, int ob, int t, int p, int q, f32x4 b, f32x4 acc) {
    const float4 a = *(const float4*)&sw[(16 * ob + p) * ld + 16 * t + 4 * q];
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b[0], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b[1], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b[2], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b[3], acc, 0, 0, 0);
    return acc;
}

// acc += M^T: output block t (inputs of the matrix), summed over the 16 outputs of block ob whose gradient is b
__device__ __forceinline__ f32x4 fm_mmT(const float* __restrict__ sw, int ld, int ob, int t, int p, int q, f32x4 b, f32x4 acc) {
    const float* a = &sw[(16 * ob + 4 * q) * ld + 16 * t + p];
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[0], b[0], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[ld], b[1], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[2 * ld], b[2], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[3 * ld], b[3], acc, 0, 0, 0);
    return acc;
}

// D layout (lane = row p, registers = columns 4 q + r) -> operand layout of a sum over rows (register s = row 4 s + q, lane = column p)
__device__ __forceinline__ f32x4 fm_transpose(f32x4 v, float* __restrict__ tb, int p, int q) {
    D3H_WAVE_SYNC();
#pragma unroll
    for (int r = 0; r < 4; ++r) tb[p * 17 + 4 * q + r] = v[r];
    D3H_WAVE_SYNC();
    f32x4 o;
#pragma unroll
    for (int s = 0; s < 4; ++s) o[s] = tb[(4 * s + q) * 17 + p];
    return o;
}

// block (ob, t) of dM += dZ^T A over the wave's 16 rows, added to the workgroup's partial sums (image layout of the stage)
__device__ __forceinline__ void fm_dw_block(f32x4 dzT, f32x4 aT, float* __restrict__ sdw, int ld, int ob, int t, int p, int q) {
    f32x4 blk = fm_zero();
#pragma unroll
    for (int s = 0; s < 4; ++s) blk = __builtin_amdgcn_mfma_f32_16x16x4f32(dzT[s], aT[s], blk, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 4; ++r) atomicAdd(&sdw[(16 * ob + 4 * q + r) * ld + 16 * t + p], blk[r]);
}

// h <- a_upto, the input of matrix `upto` (1 <= upto <= n_hidden), for this wave's 16 rows; xrow is the lane's row of x or NULL (a dead
// row: zeros).  Every wave of the workgroup calls it with the same `upto` (barriers inside); the weight image is left in use.
template <int W>
__device__ __forceinline__ void fm_forward_to(const FmPlan& P, int upto, const float* __restrict__ xrow, float* __restrict__ smem,
                                              f32x4 (&h)[W / 16], int p, int q) {
    constexpr int KB = W / 16;
    f32x4 acc[KB];
#pragma unroll
    for (int ob = 0; ob < KB; ++ob) acc[ob] = fm_zero();
    for (int s = 0; s < P.n0; ++s) {
        const float* sw = fm_weights<W>(P, s, smem);
        const int k0 = P.st_k0[s], kc = P.st_kc[s], ld = kc + FM_PAD;
        for (int tb = 0; tb < kc / 16; ++tb) {
            const int kb = k0 + 16 * tb + 4 * q;
            f32x4 xf;
#pragma unroll
            for (int r = 0; r < 4; ++r) xf[r] = (xrow && kb + r < P.n_in) ? xrow[kb + r] : 0.f;
#pragma unroll
            for (int ob = 0; ob < KB; ++ob) acc[ob] = fm_mm(sw, ld, ob, tb, p, q, xf, acc[ob]);
        }
    }
#pragma unroll
    for (int ob = 0; ob < KB; ++ob)
#pragma unroll
        for (int r = 0; r < 4; ++r) h[ob][r] = fm_act(acc[ob][r], P.act);
    for (int l = 1; l < upto; ++l) {
        const float* sw = fm_weights<W>(P, P.n0 - 1 + l, smem);
#pragma unroll
        for (int ob = 0; ob < KB; ++ob) {
            acc[ob] = fm_zero();
#pragma unroll
            for (int t = 0; t < KB; ++t) acc[ob] = fm_mm(sw, W + FM_PAD, ob, t, p, q, h[t], acc[ob]);
        }
#pragma unroll
        for (int ob = 0; ob < KB; ++ob)
#pragma unroll
            for (int r = 0; r < 4; ++r) h[ob][r] = fm_act(acc[ob][r], P.act);
    }
}

template <int W>
__global__ __launch_bounds__(256) void fusedmlp_fwd_kernel(FmPlan P, const float* __restrict__ x, int64_t n, const float* __restrict__ mask,
                                                           const float* __restrict__ out_scale, const float* __restrict__ out_bias,
                                                           float* __restrict__ out) {
    constexpr int KB = W / 16;
    D3H_DYN_SHARED(float, smem);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, p = lane & 15, q = lane >> 4;
    const int64_t ntiles = (n + 63) / 64;
    const int L = P.n_hidden, OBn = (P.n_out + 15) / 16;
    fm_preload<W>(P, smem);
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t row = tile * 64 + wave * 16 + p;
        const bool live = row < n && (!mask || mask[row] > 0.f);
        f32x4 h[KB];
        fm_forward_to<W>(P, L, live ? x + row * P.n_in : nullptr, smem, h, p, q);
        const float* sw = fm_weights<W>(P, P.n0 - 1 + L, smem);
        for (int ob = 0; ob < OBn; ++ob) {
            f32x4 z = fm_zero();
#pragma unroll
            for (int t = 0; t < KB; ++t) z = fm_mm(sw, W + FM_PAD, ob, t, p, q, h[t], z);
            if (row < n) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int c = 16 * ob + 4 * q + r;
                    if (c < P.n_out) {
                        float v = 0.f;
                        if (live) {
                            v = fm_act(z[r], P.out_act);
                            if (out_scale) v *= out_scale[c];
                            if (out_bias) v += out_bias[c];
                        }
                        out[row * P.n_out + c] = v;
                    }
                }
            }
        }
    }
}

template <int W>
__global__ __launch_bounds__(256) void fusedmlp_bwd_kernel(FmPlan P, const float* __restrict__ x, int64_t n, const float* __restrict__ mask,
                                                           const float* __restrict__ out_scale, const float* __restrict__ g_out,
                                                           float in_grad_scale, float* __restrict__ d_x) {
    constexpr int KB = W / 16;
    constexpr int LDW = W + FM_PAD;
    D3H_DYN_SHARED(float, smem);
    float* sdw = smem + P.sw_floats;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, p = lane & 15, q = lane >> 4;
    float* tb = sdw + P.sdw_floats + wave * FM_TB;
    const int64_t ntiles = (n + 63) / 64;
    const int L = P.n_hidden, n0 = P.n0, OBn = (P.n_out + 15) / 16, grp = blockIdx.y;
    // which partial sums this workgroup keeps, and the lowest matrix whose pre-activation gradient it needs
    unsigned mine = 0;
    int lo = L + 1;
    for (int s = 0; s < P.n_stages; ++s) {
        if (P.dw[P.st_layer[s]] && (P.all_groups || s == grp)) {
            mine |= 1u << s;
            lo = P.st_layer[s] < lo ? P.st_layer[s] : lo;
        }
    }
    const bool do_dx = d_x && (P.all_groups || grp == 0);
    if (do_dx) lo = 0;
    if (lo > L) return;                                    // (workgroup-uniform)
    for (int i = threadIdx.x; i < P.sdw_floats; i += 256) sdw[i] = 0.f;
    fm_preload<W>(P, smem);                                                    // (its barrier orders the zeros before any add)
    const int sL = n0 - 1 + L;
    const bool mineL = (mine >> sL) & 1u;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t row0 = tile * 64 + wave * 16, row = row0 + p;
        const bool live = row < n && (!mask || mask[row] > 0.f);
        const float* xrow = live ? x + row * P.n_in : nullptr;
        f32x4 h[KB], da[KB], dz[KB], dzT[KB];
        fm_forward_to<W>(P, L, xrow, smem, h, p, q);
#pragma unroll
        for (int t = 0; t < KB; ++t) da[t] = fm_zero();
        const float* sw = fm_weights<W>(P, sL, smem);
        // the last matrix, 16 outputs at a time: z, the gradient of z, its share of dM_L and of dA_L
        for (int ob = 0; ob < OBn; ++ob) {
            f32x4 z = fm_zero();
#pragma unroll
            for (int t = 0; t < KB; ++t) z = fm_mm(sw, LDW, ob, t, p, q, h[t], z);
            f32x4 dzb;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int c = 16 * ob + 4 * q + r;
                float gg = 0.f;
                if (live && c < P.n_out) {
                    gg = g_out[row * P.n_out + c];
                    if (out_scale) gg *= out_scale[c];
                }
                dzb[r] = gg * fm_dact(fm_act(z[r], P.out_act), P.out_act);
            }
            if (mineL) {
                const f32x4 dzbT = fm_transpose(dzb, tb, p, q);
#pragma unroll
                for (int t = 0; t < KB; ++t) fm_dw_block(dzbT, fm_transpose(h[t], tb, p, q), sdw + P.st_dwoff[sL], LDW, ob, t, p, q);
            }
            if (lo < L) {
#pragma unroll
                for (int t = 0; t < KB; ++t) da[t] = fm_mmT(sw, LDW, ob, t, p, q, dzb, da[t]);
            }
        }
        // down the hidden matrices: h holds a_{l+1}, da its gradient
        for (int l = L - 1; l >= lo; --l) {
#pragma unroll
            for (int ob = 0; ob < KB; ++ob)
#pragma unroll
                for (int r = 0; r < 4; ++r) dz[ob][r] = da[ob][r] * fm_dact(h[ob][r], P.act);
            if (l == 0) break;
            fm_forward_to<W>(P, l, xrow, smem, h, p, q);                    // a_l, the input of matrix l
            const int s = n0 - 1 + l;
            if ((mine >> s) & 1u) {
#pragma unroll
                for (int ob = 0; ob < KB; ++ob) dzT[ob] = fm_transpose(dz[ob], tb, p, q);
#pragma unroll
                for (int t = 0; t < KB; ++t) {
                    const f32x4 hT = fm_transpose(h[t], tb, p, q);
#pragma unroll
                    for (int ob = 0; ob < KB; ++ob) fm_dw_block(dzT[ob], hT, sdw + P.st_dwoff[s], LDW, ob, t, p, q);
                }
            }
            if (l > lo) {
                sw = fm_weights<W>(P, s, smem);
#pragma unroll
                for (int t = 0; t < KB; ++t) {
                    da[t] = fm_zero();
#pragma unroll
                    for (int ob = 0; ob < KB; ++ob) da[t] = fm_mmT(sw, LDW, ob, t, p, q, dz[ob], da[t]);
                }
            }
        }
        if (lo == 0) {
            // matrix 0: dz holds the gradient of its pre-activation; its input is x itself, read in either layout from memory
            bool any0 = false;
            for (int s = 0; s < n0; ++s) any0 = any0 || ((mine >> s) & 1u);
            if (any0) {
#pragma unroll
                for (int ob = 0; ob < KB; ++ob) dzT[ob] = fm_transpose(dz[ob], tb, p, q);
            }
            for (int s = 0; s < n0; ++s) {
                const bool mine0 = (mine >> s) & 1u;
                const int k0 = P.st_k0[s], kc = P.st_kc[s], ld = kc + FM_PAD;
                if (do_dx) sw = fm_weights<W>(P, s, smem);
                for (int tbk = 0; tbk < kc / 16; ++tbk) {
                    if (mine0) {
                        f32x4 xT;
                        const int k = k0 + 16 * tbk + p;
#pragma unroll
                        for (int s4 = 0; s4 < 4; ++s4) {
                            const int64_t r2 = row0 + 4 * s4 + q;
                            const bool live2 = r2 < n && k < P.n_in && (!mask || mask[r2] > 0.f);
                            xT[s4] = live2 ? x[r2 * P.n_in + k] : 0.f;
                        }
#pragma unroll
                        for (int ob = 0; ob < KB; ++ob) fm_dw_block(dzT[ob], xT, sdw + P.st_dwoff[s], ld, ob, tbk, p, q);
                    }
                    if (do_dx) {
                        f32x4 acc = fm_zero();
#pragma unroll
                        for (int ob = 0; ob < KB; ++ob) acc = fm_mmT(sw, ld, ob, tbk, p, q, dz[ob], acc);
                        if (row < n) {
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                const int k = k0 + 16 * tbk + 4 * q + r;
                                if (k < P.n_in) d_x[row * P.n_in + k] = live ? acc[r] * in_grad_scale : 0.f;
                            }
                        }
                    }
                }
            }
        }
    }
    // flush the workgroup's partial sums, once
    __syncthreads();
    for (int s = 0; s < P.n_stages; ++s) {
        if (!((mine >> s) & 1u)) continue;
        const int l = P.st_layer[s], k0 = P.st_k0[s], kc = P.st_kc[s], ld = kc + FM_PAD;
        const int fi = fm_fan_in<W>(P, l), fo = fm_fan_out<W>(P, l);
        float* __restrict__ dst = P.dw[l];
        const float* __restrict__ src = sdw + P.st_dwoff[s];
        for (int idx = threadIdx.x; idx < fo * kc; idx += 256) {
            const int o = idx / kc, k = idx - o * kc;
            if (k0 + k < fi) atomicAdd(&dst[(size_t)o * fi + k0 + k], src[o * ld + k]);
        }
    }
}

bool fm_ok_ptr(const void* p) { return ((uintptr_t)p & 3u) == 0; }

// shape checks and the stage table; rc D3H_OK or D3H_ERR_ARG
int fm_make_plan(int n_in, int width, int n_hidden, int n_out, int act, int out_act, const float* const* w, FmPlan* out) {
    if (width != 16 && width != 32 && width != 64 && width != 128) return D3H_ERR_ARG;
    if (n_hidden < 1 || n_hidden > 8 || n_in < 1 || n_in > 256 || n_out < 1 || n_out > 128) return D3H_ERR_ARG;
    if (act < 0 || act >= FM_NACT || out_act < 0 || out_act >= FM_NACT || !w) return D3H_ERR_ARG;
    FmPlan P = {};
    P.n_in = n_in; P.n_out = n_out; P.n_hidden = n_hidden; P.width = width; P.act = act; P.out_act = out_act;
    P.all_groups = 1;
    int ns = 0, sw = 0, tot = 0;
    const int K0 = (n_in + 15) & ~15;
    for (int k0 = 0; k0 < K0; k0 += FM_KC) {
        P.st_layer[ns] = 0; P.st_k0[ns] = k0; P.st_kc[ns] = K0 - k0 < FM_KC ? K0 - k0 : FM_KC;
        ++ns;
    }
    P.n0 = ns;
    for (int l = 1; l <= n_hidden; ++l) {
        P.st_layer[ns] = l; P.st_k0[ns] = 0; P.st_kc[ns] = width;
        ++ns;
    }
    P.n_stages = ns;
    for (int s = 0; s < ns; ++s) {
        const int fo = P.st_layer[s] == n_hidden ? n_out : width;
        const int fl = ((fo + 15) & ~15) * (P.st_kc[s] + FM_PAD);
        sw = fl > sw ? fl : sw;
        tot += fl;
    }
    P.sw_max = sw;
    P.sw_total = tot;
    for (int l = 0; l <= n_hidden; ++l) {
        if (!w[l] || !fm_ok_ptr(w[l])) return D3H_ERR_ARG;
        P.w[l] = w[l];
    }
    *out = P;
    return D3H_OK;
}


int fm_stage_floats(const FmPlan& P, int, int s) {
    const int fo = P.st_layer[s] == P.n_hidden ? P.n_out : P.width;
    return ((fo + 15) & ~15) * (P.st_kc[s] + FM_PAD);
}

int fm_grid(int64_t n, int lds_bytes, int max_cus) {
    const int64_t ntiles = (n + 63) / 64;
    int per_cu = FM_LDS_MAX / (lds_bytes > 0 ? lds_bytes : 1);
    per_cu = per_cu < 1 ? 1 : (per_cu > 4 ? 4 : per_cu);
    const int64_t cap = max_cus > 0 ? (int64_t)max_cus : (int64_t)256 * per_cu;
    return (int)(ntiles < cap ? ntiles : cap);
}

// the images side by side (resident) or one at a time
void fm_place_images(FmPlan& P, bool resident) {
    P.resident = resident ? 1 : 0;
    P.sw_floats = resident ? P.sw_total : P.sw_max;
    int off = 0;
    for (int st = 0; st < P.n_stages; ++st) {
        P.st_swoff[st] = resident ? off : 0;
        off += fm_stage_floats(P, 0, st);
    }
}

template <int W>
int fm_launch_fwd(FmPlan P, const float* x, int64_t n, const float* mask, const float* out_scale, const float* out_bias, float* out,
                  int max_cus, hipStream_t s) {
    fm_place_images(P, P.sw_total * 4 <= FM_LDS_RESIDENT);
    const int lds = P.sw_floats * 4;
#ifndef D3H_EMULATED
    if (lds > 48 * 1024 && hipFuncSetAttribute((const void*)fusedmlp_fwd_kernel<W>, hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess)
        (void)hipGetLastError();            // (a runtime that needs no opt-in may refuse the attribute: the launch check below decides)
#endif
    hipLaunchKernelGGL((fusedmlp_fwd_kernel<W>), dim3((unsigned)fm_grid(n, lds, max_cus)), dim3(256), (size_t)lds, s, P, x, n, mask, out_scale,
                       out_bias, out);
    D3H_LAUNCH_CHECK();
    return D3H_OK;
}

template <int W>
int fm_launch_bwd(FmPlan P, const float* x, int64_t n, const float* mask, const float* out_scale, const float* g_out, float in_grad_scale,
                  float* d_x, int max_cus, hipStream_t s) {
    // the partial sums: all stages next to the weight image when they fit, else one stage per grid slice
    int total = 0, largest = 0, wanted = 0;
    for (int st = 0; st < P.n_stages; ++st) {
        P.st_dwoff[st] = total;
        if (!P.dw[P.st_layer[st]]) continue;
        const int fl = fm_stage_floats(P, W, st);
        total += fl;
        largest = fl > largest ? fl : largest;
        ++wanted;
    }
    int groups = 1;
    P.all_groups = 1;
    P.sdw_floats = total;
    fm_place_images(P, (P.sw_total + total + 4 * FM_TB) * 4 <= FM_LDS_RESIDENT);
    if ((P.sw_floats + total + 4 * FM_TB) * 4 > FM_LDS_MAX) {
        P.all_groups = 0;
        P.sdw_floats = largest;
        for (int st = 0; st < P.n_stages; ++st) P.st_dwoff[st] = 0;
        groups = P.n_stages;
    }
    (void)wanted;
    const int lds = (P.sw_floats + P.sdw_floats + 4 * FM_TB) * 4;
    if (lds > FM_LDS_MAX) return D3H_ERR_ARG;
#ifndef D3H_EMULATED
    if (lds > 48 * 1024 && hipFuncSetAttribute((const void*)fusedmlp_bwd_kernel<W>, hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess)
        (void)hipGetLastError();
#endif
    hipLaunchKernelGGL((fusedmlp_bwd_kernel<W>), dim3((unsigned)fm_grid(n, lds, max_cus), (unsigned)groups), dim3(256), (size_t)lds, s, P, x, n,
                       mask, out_scale, g_out, in_grad_scale, d_x);
    D3H_LAUNCH_CHECK();
    return D3H_OK;
}

#define FM_DISPATCH(FN, ...)                         \
    switch (width) {                                 \
        case 16: return FN<16>(__VA_ARGS__);         \
        case 32: return FN<32>(__VA_ARGS__);         \
        case 64: return FN<64>(__VA_ARGS__);         \
        default: return FN<128>(__VA_ARGS__);        \
    }

}  // namespace

// ------------------------------------------------------------------------------------------------
// C ABI   (bias-free MLP n_in -> width -> ... -> width -> n_out; width 16 | 32 | 64 | 128; n_hidden_layers 1..8, i.e. n_hidden_layers + 1
//          matrices in nn.Linear layout [fan_out][fan_in]; n_in 1..256; n_out 1..128; act / out_act: 0 None, 1 ReLU, 2 LeakyReLU (0.01),
//          3 Sigmoid, 4 Tanh, 5 Softplus, 6 Exponential)
// ------------------------------------------------------------------------------------------------
// x [n][n_in]; w: HOST array of n_hidden_layers + 1 device pointers; mask NULL or [n]: rows with mask <= 0 give a zero row; out_scale /
// out_bias NULL or [n_out]: out [n][n_out] = out_act(z) * out_scale[c] + out_bias[c], overwritten.  max_cus > 0: exactly min(tiles of 64
// rows, max_cus) workgroups; 0: the whole chip.  n == 0 returns without a launch; an unsupported shape or activation, a NULL or misaligned
// pointer returns an argument error before any launch.
extern "C" int d3h_fusedmlp_fwd(const float* x, int64_t n, int n_in, int width, int n_hidden_layers, int n_out, int act, int out_act,
                                const float* const* w, const float* mask, const float* out_scale, const float* out_bias, float* out, int max_cus,
                                void* stream) {
    FmPlan P;
    if (fm_make_plan(n_in, width, n_hidden_layers, n_out, act, out_act, w, &P) != D3H_OK) return D3H_ERR_ARG;
    if (n < 0 || n > ((int64_t)1 << 36) || max_cus < 0) return D3H_ERR_ARG;
    if (!fm_ok_ptr(x) || !fm_ok_ptr(mask) || !fm_ok_ptr(out_scale) || !fm_ok_ptr(out_bias) || !fm_ok_ptr(out)) return D3H_ERR_ARG;
    if (n == 0) return D3H_OK;
    if (!x || !out) return D3H_ERR_ARG;
    FM_DISPATCH(fm_launch_fwd, P, x, n, mask, out_scale, out_bias, out, max_cus, (hipStream_t)stream);
}

// g_out [n][n_out]; d_x NULL or [n][n_in], OVERWRITTEN with in_grad_scale * dL/dx (zero rows where mask <= 0); d_w NULL or a HOST array
// of n_hidden_layers + 1 device pointers, each NULL or [fan_out][fan_in], ACCUMULATED (out_scale enters, out_bias does not; masked rows
// add nothing).  Reads x, the weights and g_out only: the forward of each tile is recomputed.  The partial sums of d_w are kept per
// workgroup and flushed once with float atomics: the last bits depend on the order of arrival.  First order only.
extern "C" int d3h_fusedmlp_bwd(const float* x, int64_t n, int n_in, int width, int n_hidden_layers, int n_out, int act, int out_act,
                                const float* const* w, const float* mask, const float* out_scale, const float* g_out, float in_grad_scale,
                                float* d_x, float* const* d_w, int max_cus, void* stream) {
    FmPlan P;
    if (fm_make_plan(n_in, width, n_hidden_layers, n_out, act, out_act, w, &P) != D3H_OK) return D3H_ERR_ARG;
    if (n < 0 || n > ((int64_t)1 << 36) || max_cus < 0) return D3H_ERR_ARG;
    if (!fm_ok_ptr(x) || !fm_ok_ptr(mask) || !fm_ok_ptr(out_scale) || !fm_ok_ptr(g_out) || !fm_ok_ptr(d_x)) return D3H_ERR_ARG;
    bool any = d_x != nullptr;
    for (int l = 0; d_w && l <= n_hidden_layers; ++l) {
        if (!fm_ok_ptr(d_w[l])) return D3H_ERR_ARG;
        P.dw[l] = d_w[l];
        any = any || d_w[l] != nullptr;
    }
    if (n == 0 || !any) return D3H_OK;
    if (!x || !g_out) return D3H_ERR_ARG;
    FM_DISPATCH(fm_launch_bwd, P, x, n, mask, out_scale, g_out, in_grad_scale, d_x, max_cus, (hipStream_t)stream);
}
