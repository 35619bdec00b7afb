// gridenc.hip -- general multiresolution grid encoding (tiny-cuda-nn "HashGrid" / "DenseGrid"), forward and backward, for gfx950.
//
// The configurations of tcnn.Encoding that csrc/texmlp.hip does not build: any level count, 2-D and 3-D inputs, 1 / 2 / 4 / 8 features per
// entry, hashed levels, smoothstep interpolation.  tiny-cuda-nn is an un-vendored dependency of the reference (README.md:30): "parity
// unpinned", the semantics restate its published algorithm (recalled; the contract is the docstring of d3h/gridenc.py, pinned against the
// float64 restatement tests/gridenc_cases.py:ref_encode and, on the reference configuration, against oracle/texmlp.py).
//   level l: scale = exp2f(l log2f(s)) B - 1, res = ceil(scale) + 1, n_l = round_up(res^D, 8) entries (Hash: at most 2^T);
//   p = fmaf(x, scale, 0.5); the 2^D corners of floor(p), corner bit d = bit d of the corner number;
//   entry = (dense: sum_d q_d res^d | hashed, when res^D > n_l: q_0 ^ q_1 2654435761 ^ q_2 805459861) % n_l, all in uint32.
//
// Bounds.  Every table access, load or atomic, goes through entry_of(), whose last operation reduces an arbitrary uint32 `% n_l` (or
// `& (n_l - 1)` when n_l is a power of two, the same value), with 1 <= n_l; the address is table + (offset_l + entry) * F with
// offset_l + n_l <= sum(n_l), and the entry points refuse a table whose length is not sum(n_l) * F.  The corner coordinate is formed from
// floorf(p) clamped to [-2^31, 2^31 - 128] (fmaxf / fminf return the other operand for a NaN) BEFORE the conversion to an integer, so the
// conversion is defined for every float32 input, infinities and NaN included, and everything after it is wrapping unsigned arithmetic.
// A point outside [0, 1]^D therefore reads and adds inside the table whatever its value (an unspecified row, never another allocation);
// the clamp cannot change a point inside [0, 1]^D (there floor(p) <= scale + 0.5 < 2^24).  Rows of x / g / out / d_x are touched only for i < n.
//
// MI355X design ("general grid encoding"):
//  - level-major: the level is the slow grid index (blockIdx.y) and a thread owns one point of one level, so the workgroups in flight
//    gather from ONE level's slice (at most 2^T F 4 bytes: 4 MB at T = 19, 16 MB at T = 21 for F = 2) instead of from the whole 50-180 MB
//    table: a slice sits in the Infinity Cache, a coarse one in the XCDs' L2s;
//  - the F features of an entry are one vector load (4 / 8 / 16 / 2 x 16 bytes); all 2^D corner loads are issued before the first is used
//    (the indices are computed first, the loads fill an array, the blend follows);
//  - D, F and the interpolation are template parameters (16 instantiations per kernel), the level count is a launch dimension, hashed or
//    dense is a wave-uniform branch on a kernel argument;
//  - the table gradient is a scatter of fp32 atomics (global_atomic_add_f32, no compare-and-swap loop).  Lanes of a wave whose points sit
//    in the same cell (coarse levels under pixel-coherent input) are summed with a segmented wave scan and added once per run, as
//    texmlp_bwd_kernel<1> does; a wave without two adjacent lanes in one cell (random points, fine levels) skips the scan;
//  - the position gradient needs the corner features again (a second gather) and is summed over the levels with L atomics per
//    coordinate onto a zero-filled d_x (contiguous 4 D-byte rows per lane).
#include "d3h_common.h"

namespace {

constexpr int GE_MAXL = 32;
constexpr uint32_t GE_PRIME1 = 2654435761u, GE_PRIME2 = 805459861u;

struct GeLayout {
    float scale[GE_MAXL];
    uint32_t res[GE_MAXL];
    uint32_t offset[GE_MAXL];    // in entries
    uint32_t size[GE_MAXL];      // n_l
    uint32_t hashed;             // bit l: level l is hashed
    int n_levels;
    int64_t total;               // sum(n_l)
};

// rc: 0, D3H_ERR_ARG, or -2: the table would have 2^31 entries or more
int ge_make_layout(int n_dims, int n_levels, int n_features, int log2_hashmap_size, int base_res, double per_level_scale, int grid_type,
                   GeLayout* out) {
    if (n_dims < 2 || n_dims > 3 || n_levels < 1 || n_levels > GE_MAXL) return D3H_ERR_ARG;
    if (n_features != 1 && n_features != 2 && n_features != 4 && n_features != 8) return D3H_ERR_ARG;
    if (grid_type != 0 && grid_type != 1) return D3H_ERR_ARG;
    if (base_res < 1 || !(per_level_scale > 0.0) || log2_hashmap_size < 0 || log2_hashmap_size > 31) return D3H_ERR_ARG;
    GeLayout g;
    g.hashed = 0;
    g.n_levels = n_levels;
    int64_t off = 0;
    const int64_t cap = (int64_t)1 << log2_hashmap_size;
    for (int l = 0; l < GE_MAXL; ++l) { g.scale[l] = 0.f; g.res[l] = 1; g.offset[l] = 0; g.size[l] = 1; }
    for (int l = 0; l < n_levels; ++l) {
        const float scale = exp2f((float)l * log2f((float)per_level_scale)) * (float)base_res - 1.0f;
        if (!(scale >= 0.f) || !(scale < 1.0e9f)) return D3H_ERR_ARG;
        const int64_t res = (int64_t)ceilf(scale) + 1;
        double cells = 1.0;
        for (int d = 0; d < n_dims; ++d) cells *= (double)res;
        int64_t n_l;
        if (cells >= 2147483648.0) {               // res^D itself is 2^31 or more
            if (grid_type == 1) return -2;
            n_l = cap;
            g.hashed |= 1u << l;
        } else {
            int64_t cnt = 1;
            for (int d = 0; d < n_dims; ++d) cnt *= res;
            n_l = (cnt + 7) / 8 * 8;
            if (grid_type == 0 && n_l > cap) n_l = cap;
            if (cnt > n_l) g.hashed |= 1u << l;
        }
        off += n_l;
        if (off >= ((int64_t)1 << 31)) return -2;
        g.scale[l] = scale;
        g.res[l] = (uint32_t)res;
        g.offset[l] = (uint32_t)(off - n_l);
        g.size[l] = (uint32_t)n_l;
    }
    g.total = off;
    *out = g;
    return D3H_OK;
}

template <int F> struct GeVec { float v[F]; };

template <int F> __device__ __forceinline__ GeVec<F> ge_load(const float* __restrict__ p) {
    GeVec<F> r;
    if constexpr (F == 1) {
        r.v[0] = p[0];
    } else if constexpr (F == 2) {
        const float2 t = *(const float2*)p;
        r.v[0] = t.x; r.v[1] = t.y;
    } else if constexpr (F == 4) {
        const float4 t = *(const float4*)p;
        r.v[0] = t.x; r.v[1] = t.y; r.v[2] = t.z; r.v[3] = t.w;
    } else {
        const float4 a = ((const float4*)p)[0], b = ((const float4*)p)[1];
        r.v[0] = a.x; r.v[1] = a.y; r.v[2] = a.z; r.v[3] = a.w;
        r.v[4] = b.x; r.v[5] = b.y; r.v[6] = b.z; r.v[7] = b.w;
    }
    return r;
}

template <int F> __device__ __forceinline__ void ge_store(float* __restrict__ p, const GeVec<F>& r) {
    if constexpr (F == 1) {
        p[0] = r.v[0];
    } else if constexpr (F == 2) {
        *(float2*)p = make_float2(r.v[0], r.v[1]);
    } else if constexpr (F == 4) {
        *(float4*)p = make_float4(r.v[0], r.v[1], r.v[2], r.v[3]);
    } else {
        ((float4*)p)[0] = make_float4(r.v[0], r.v[1], r.v[2], r.v[3]);
        ((float4*)p)[1] = make_float4(r.v[4], r.v[5], r.v[6], r.v[7]);
    }
}

struct GeLevel {
    float scale;
    uint32_t res, size;
    bool hashed, pow2;
};

__device__ __forceinline__ GeLevel ge_level(const GeLayout& lay, int l) {
    GeLevel lv;
    lv.scale = lay.scale[l];
    lv.res = lay.res[l];
    lv.size = lay.size[l];
    lv.hashed = (lay.hashed >> l) & 1u;
    lv.pow2 = (lv.size & (lv.size - 1u)) == 0u;
    return lv;
}

// cell and fraction of a point on a level (see "Bounds" above for the clamp)
template <int D> __device__ __forceinline__ void ge_locate(const float* __restrict__ xp, float scale, uint32_t (&q)[D], float (&fr)[D]) {
#pragma unroll
    for (int d = 0; d < D; ++d) {
        const float p = fmaf(xp[d], scale, 0.5f);
        const float fl = floorf(p);
        fr[d] = p - fl;
        const float c = fminf(fmaxf(fl, -2147483648.0f), 2147483520.0f);
        q[d] = (uint32_t)(int32_t)c;
    }
}

// table entry of corner `c` of cell q: ALWAYS < lv.size
template <int D> __device__ __forceinline__ uint32_t entry_of(const GeLevel& lv, const uint32_t (&q)[D], int c) {
    uint32_t idx = 0;
    if (lv.hashed) {
        idx = q[0] + (uint32_t)(c & 1);
        idx ^= (q[1] + (uint32_t)((c >> 1) & 1)) * GE_PRIME1;
        if constexpr (D == 3) idx ^= (q[2] + (uint32_t)((c >> 2) & 1)) * GE_PRIME2;
    } else {
        uint32_t stride = 1;
#pragma unroll
        for (int d = 0; d < D; ++d) {
            idx += (q[d] + (uint32_t)((c >> d) & 1)) * stride;
            stride *= lv.res;
        }
    }
    return lv.pow2 ? (idx & (lv.size - 1u)) : (idx % lv.size);
}

template <int D, bool SMOOTH> __device__ __forceinline__ void ge_weights(const float (&fr)[D], float (&w)[D], float (&dw)[D]) {
#pragma unroll
    for (int d = 0; d < D; ++d) {
        if (SMOOTH) {
            w[d] = fr[d] * fr[d] * (3.f - 2.f * fr[d]);
            dw[d] = 6.f * fr[d] * (1.f - fr[d]);
        } else {
            w[d] = fr[d];
            dw[d] = 1.f;
        }
    }
}

template <int D> __device__ __forceinline__ float ge_corner_weight(const float (&w)[D], int c) {
    float r = 1.f;
#pragma unroll
    for (int d = 0; d < D; ++d) r *= ((c >> d) & 1) ? w[d] : (1.f - w[d]);
    return r;
}

template <int D, int F, bool SMOOTH>
__global__ __launch_bounds__(256) void gridenc_fwd_kernel(GeLayout lay, const float* __restrict__ x, const float* __restrict__ table, int64_t n,
                                                          float* __restrict__ out) {
    constexpr int NC = 1 << D;
    const int l = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const GeLevel lv = ge_level(lay, l);
    uint32_t q[D];
    float fr[D], w[D], dw[D];
    ge_locate<D>(x + i * D, lv.scale, q, fr);
    ge_weights<D, SMOOTH>(fr, w, dw);
    const float* tab = table + (size_t)lay.offset[l] * F;
    uint32_t idx[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) idx[c] = entry_of<D>(lv, q, c);
    GeVec<F> v[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) v[c] = ge_load<F>(tab + (size_t)idx[c] * F);
    GeVec<F> acc;
#pragma unroll
    for (int f = 0; f < F; ++f) acc.v[f] = 0.f;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const float wc = ge_corner_weight<D>(w, c);
#pragma unroll
        for (int f = 0; f < F; ++f) acc.v[f] = fmaf(wc, v[c].v[f], acc.v[f]);
    }
    ge_store<F>(out + (size_t)i * ((size_t)lay.n_levels * F) + (size_t)l * F, acc);
}

// d_table (accumulated) and / or d_x (accumulated) of one level per workgroup row; every lane of a wave reaches every wave-level operation
template <int D, int F, bool SMOOTH>
__global__ __launch_bounds__(256) void gridenc_bwd_kernel(GeLayout lay, const float* __restrict__ x, const float* __restrict__ table,
                                                          const float* __restrict__ g, int64_t n, float* __restrict__ d_table,
                                                          float* __restrict__ d_x) {
    constexpr int NC = 1 << D;
    const int l = blockIdx.y;
    const int lane = threadIdx.x & 63;
    const int64_t i0 = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool active = i0 < n;
    const int64_t i = active ? i0 : n - 1;            // an idle lane of the last workgroup re-reads the last point and adds nothing
    const GeLevel lv = ge_level(lay, l);
    uint32_t q[D];
    float fr[D], w[D], dw[D];
    ge_locate<D>(x + i * D, lv.scale, q, fr);
    ge_weights<D, SMOOTH>(fr, w, dw);
    GeVec<F> gv = ge_load<F>(g + (size_t)i * ((size_t)lay.n_levels * F) + (size_t)l * F);
    if (!active) {
#pragma unroll
        for (int f = 0; f < F; ++f) gv.v[f] = 0.f;
    }
    uint32_t idx[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) idx[c] = entry_of<D>(lv, q, c);
    if (d_table) {
        float* dtab = d_table + (size_t)lay.offset[l] * F;
        // runs of adjacent lanes in the same cell (exact: every coordinate is compared, not a combined key)
        bool head = lane == 0;
        {
            const int pa = __shfl_up((int)active, 1);
            head = head || (pa != (int)active);
#pragma unroll
            for (int d = 0; d < D; ++d) {
                const int pq = __shfl_up((int)q[d], 1);
                head = head || (pq != (int)q[d]);
            }
        }
        const unsigned long long heads = __ballot(head);
        if (__popcll(heads) == 64) {
            // no two neighbours share a cell: one atomic per lane, corner and feature
            if (active) {
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    const float wc = ge_corner_weight<D>(w, c);
#pragma unroll
                    for (int f = 0; f < F; ++f) atomicAdd(&dtab[(size_t)idx[c] * F + f], wc * gv.v[f]);
                }
            }
        } else {
            const int start = 63 - __clzll((long long)(heads & (~0ull >> (63 - lane))));
            const bool tail = (lane == 63) || ((heads >> (lane + 1)) & 1ull);
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const float wc = ge_corner_weight<D>(w, c);
#pragma unroll
                for (int f = 0; f < F; ++f) {
                    const float s = d3h_seg_sum(wc * gv.v[f], lane, start);
                    if (tail && active) atomicAdd(&dtab[(size_t)idx[c] * F + f], s);
                }
            }
        }
    }
    if (d_x && active) {
        const float* tab = table + (size_t)lay.offset[l] * F;
        GeVec<F> v[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) v[c] = ge_load<F>(tab + (size_t)idx[c] * F);
        float dot[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            float a = 0.f;
#pragma unroll
            for (int f = 0; f < F; ++f) a = fmaf(v[c].v[f], gv.v[f], a);
            dot[c] = a;
        }
#pragma unroll
        for (int d = 0; d < D; ++d) {
            float a = 0.f;
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                float t = dot[c];
#pragma unroll
                for (int e = 0; e < D; ++e) {
                    if (e != d) t *= ((c >> e) & 1) ? w[e] : (1.f - w[e]);
                }
                a += ((c >> d) & 1) ? t : -t;
            }
            atomicAdd(&d_x[i * D + d], lv.scale * dw[d] * a);
        }
    }
}

template <int D, int F, bool SMOOTH>
void ge_launch_fwd(const GeLayout& lay, const float* x, const float* table, int64_t n, float* out, hipStream_t s) {
    const dim3 grid((unsigned)((n + 255) / 256), (unsigned)lay.n_levels);
    hipLaunchKernelGGL((gridenc_fwd_kernel<D, F, SMOOTH>), grid, dim3(256), 0, s, lay, x, table, n, out);
}

template <int D, int F, bool SMOOTH>
void ge_launch_bwd(const GeLayout& lay, const float* x, const float* table, const float* g, int64_t n, float* d_table, float* d_x, hipStream_t s) {
    const dim3 grid((unsigned)((n + 255) / 256), (unsigned)lay.n_levels);
    hipLaunchKernelGGL((gridenc_bwd_kernel<D, F, SMOOTH>), grid, dim3(256), 0, s, lay, x, table, g, n, d_table, d_x);
}

#define GE_DISPATCH_F(FN, D_, S_, ...)                 \
    switch (n_features) {                              \
        case 1: FN<D_, 1, S_>(__VA_ARGS__); break;     \
        case 2: FN<D_, 2, S_>(__VA_ARGS__); break;     \
        case 4: FN<D_, 4, S_>(__VA_ARGS__); break;     \
        default: FN<D_, 8, S_>(__VA_ARGS__); break;    \
    }
#define GE_DISPATCH(FN, ...)                                            \
    do {                                                                \
        if (n_dims == 2) {                                              \
            if (interpolation) { GE_DISPATCH_F(FN, 2, true, __VA_ARGS__) } \
            else { GE_DISPATCH_F(FN, 2, false, __VA_ARGS__) }           \
        } else {                                                        \
            if (interpolation) { GE_DISPATCH_F(FN, 3, true, __VA_ARGS__) } \
            else { GE_DISPATCH_F(FN, 3, false, __VA_ARGS__) }           \
        }                                                               \
    } while (0)

bool ge_aligned(const void* p, int n_features) { return ((uintptr_t)p % (uintptr_t)(4 * n_features)) == 0; }

}  // namespace

// ------------------------------------------------------------------------------------------------
// C ABI   (grid_type: 0 = Hash, 1 = Dense; interpolation: 0 = Linear, 1 = Smoothstep; n_dims 2 | 3; n_features 1 | 2 | 4 | 8;
//          n_levels 1..32; the table is sum(n_l) * n_features floats, entry-major inside a level)
// ------------------------------------------------------------------------------------------------
// HOST only, no launch: the per-level layout into HOST arrays of n_levels elements each (any may be NULL) and the total entry count.
// Returns -2 when the table would have 2^31 entries or more.
extern "C" int d3h_gridenc_layout(int n_dims, int n_levels, int n_features, int log2_hashmap_size, int base_res, double per_level_scale,
                                  int grid_type, float* scale, int* res, int64_t* offset, int64_t* size, int* hashed, int64_t* total_entries) {
    GeLayout lay;
    const int rc = ge_make_layout(n_dims, n_levels, n_features, log2_hashmap_size, base_res, per_level_scale, grid_type, &lay);
    if (rc != D3H_OK) return rc;
    for (int l = 0; l < n_levels; ++l) {
        if (scale) scale[l] = lay.scale[l];
        if (res) res[l] = (int)lay.res[l];
        if (offset) offset[l] = (int64_t)lay.offset[l];
        if (size) size[l] = (int64_t)lay.size[l];
        if (hashed) hashed[l] = (int)((lay.hashed >> l) & 1u);
    }
    if (total_entries) *total_entries = lay.total;
    return D3H_OK;
}

// x [n][n_dims] (expected in [0, 1], NOT clamped; any float32 value stays inside the table); table [table_floats]; out [n][n_levels * n_features]
// overwritten, column l * n_features + f.  table and out must be aligned to 4 * n_features bytes.
extern "C" int d3h_gridenc_fwd(const float* x, const float* table, int64_t table_floats, int64_t n, int n_dims, int n_levels, int n_features,
                               int log2_hashmap_size, int base_res, double per_level_scale, int grid_type, int interpolation, float* out,
                               void* stream) {
    GeLayout lay;
    if (ge_make_layout(n_dims, n_levels, n_features, log2_hashmap_size, base_res, per_level_scale, grid_type, &lay) != D3H_OK) return D3H_ERR_ARG;
    if (n < 0 || n > ((int64_t)1 << 38) || (interpolation != 0 && interpolation != 1) || table_floats != lay.total * n_features) return D3H_ERR_ARG;
    if (n == 0) return D3H_OK;
    if (!x || !table || !out || !ge_aligned(table, n_features) || !ge_aligned(out, n_features)) return D3H_ERR_ARG;
    GE_DISPATCH(ge_launch_fwd, lay, x, table, n, out, (hipStream_t)stream);
    D3H_LAUNCH_CHECK();
    return D3H_OK;
}

// g_out [n][n_levels * n_features]; d_table [table_floats] and d_x [n][n_dims] are ACCUMULATED (caller zero-fills); either may be NULL and
// its work is skipped (table may be NULL when d_x is).  First order only.  table, g_out and d_table aligned to 4 * n_features bytes.
extern "C" int d3h_gridenc_bwd(const float* x, const float* table, int64_t table_floats, const float* g_out, int64_t n, int n_dims, int n_levels,
                               int n_features, int log2_hashmap_size, int base_res, double per_level_scale, int grid_type, int interpolation,
                               float* d_table, float* d_x, void* stream) {
    GeLayout lay;
    if (ge_make_layout(n_dims, n_levels, n_features, log2_hashmap_size, base_res, per_level_scale, grid_type, &lay) != D3H_OK) return D3H_ERR_ARG;
    if (n < 0 || n > ((int64_t)1 << 38) || (interpolation != 0 && interpolation != 1) || table_floats != lay.total * n_features) return D3H_ERR_ARG;
    if (n == 0 || (!d_table && !d_x)) return D3H_OK;
    if (!x || !g_out || (d_x && !table) || !ge_aligned(g_out, n_features) || !ge_aligned(d_table, n_features) || !ge_aligned(table, n_features))
        return D3H_ERR_ARG;
    GE_DISPATCH(ge_launch_bwd, lay, x, table, g_out, n, d_table, d_x, (hipStream_t)stream);
    D3H_LAUNCH_CHECK();
    return D3H_OK;
}
