// d3h_bcast.h -- [B,H,W,C] tensors that may be broadcast along any of B / H / W (element stride 0), as the reference plugin's tensor wrapper
// allows (render/renderutils/c_src/tensor.h:20-92).  Shared by the per-pixel kernels of image_ops.hip (prepare_shading_normal) and bsdf.hip.
#pragma once
#include "d3h_vec.h"

namespace {

struct Bc { const float* p; long long sb, sh, sw; };
__device__ __forceinline__ const float* bc_at(const Bc& t, int b, int y, int x) { return t.p + b * t.sb + y * t.sh + x * t.sw; }
__device__ __forceinline__ V3 fetch(const Bc& t, int b, int y, int x) { return ld3(bc_at(t, b, y, x)); }
__device__ __forceinline__ float fetch1(const Bc& t, int b, int y, int x) { return *bc_at(t, b, y, x); }

// strides[3 k .. 3 k + 2]: the (b, h, w) element strides of tensor k, as d3h/imgops.py:_bc_strides lays them out
static inline Bc bc_make(const float* p, const int64_t* strides, int k) {
    Bc t;
    t.p = p; t.sb = strides[3 * k]; t.sh = strides[3 * k + 1]; t.sw = strides[3 * k + 2];
    return t;
}

// pixel i of a [B][H][W] sweep -> (b, y, x)
__device__ __forceinline__ void bc_pixel(size_t i, int H, int W, int& b, int& y, int& x) {
    b = (int)(i / ((size_t)H * W));
    int rem = (int)(i % ((size_t)H * W));
    y = rem / W; x = rem % W;
}

}  // namespace
