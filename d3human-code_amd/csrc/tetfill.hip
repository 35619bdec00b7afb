// tetfill.hip -- the tetrahedra of a lattice on the inside of the zero set of a vertex field ("a lattice clipped by the linear interpolant of
// the signed distance"), gfx950.
//
// Replaces script/get_tet_smpl.py:9-27 (get_tet_mesh: tetgen's constrained Delaunay mesh of the SMPL-X template, behind pyvista) as used by
// geometry/hmsdf.py:239-249 at start-up.  It does not reproduce tetgen: the result is the part of a tet grid on one side of the piecewise linear
// field, its boundary is the marching-tets surface of that field and its cut vertices ARE marching tets' watertight vertices (the expression of
// mt_emit_verts, marching_tets.hip, operation by operation: same bits, same order).  Start-up code, three launches, no claim about speed.
//
// Side test (marching tets' own, mt_count_edges): occ = sdf > 0; a vertex is INSIDE when !(sdf > 0).  A NaN sets bit 1 of the error word.
//
// Output vertices: the inside lattice vertices in lattice order (id = rank among inside vertices), then one cut vertex per sign-changing edge
// in the order of the sorted-unique edge list (id = n_inside + rank).  Both ranks are monotone and every lattice id is below every cut id.
//
// Output tets: parents in tet order, children in the order below, at the exclusive scan of the child counts 0, 1, 3, 3, 1 for 0, 1, 2, 3, 4
// inside corners.  I / O = the inside / outside corners in the parent's corner order, c(i,o) = the cut vertex on edge (i,o):
//   4 inside   the parent
//   1 inside   (i, c(i,o0), c(i,o1), c(i,o2))
//   2 inside   prism [i0, c(i0,o0), c(i0,o1) | i1, c(i1,o0), c(i1,o1)]
//   3 inside   prism [i0, i1, i2 | c(i0,o), c(i1,o), c(i2,o)]
// A prism [P0 P1 P2 | P3 P4 P5] (Pk pairs with Pk+3) is split smallest id first (Dompierre et al., "How to subdivide pyramids, prisms and
// hexahedra into tetrahedra", 1999): if the smallest of the six ids is in the second triangle the triangles are swapped; both triangles are
// rotated together until it is V0; then
//   min(V1,V5) < min(V2,V4):  (V0,V1,V2,V5) (V0,V1,V5,V4) (V0,V4,V5,V3)
//   otherwise:                (V0,V1,V2,V4) (V0,V4,V2,V5) (V0,V4,V5,V3)
// Two parents that share a cut quad see the same four ids on it, so both cut it along the diagonal through its smallest id.
//
// Orientation is combinatorial.  With q = (I ascending, O ascending) as a permutation of the corners (0,1,2,3), every child above has the
// orientation of the parent times the sign of q, times -1 if the prism's triangles were swapped (the rotation and both Dompierre splits keep
// it).  Sign of q by inside mask (bit k = corner k inside), 1 = odd:
//   mask    0 1 2 3 4 5 6 7 8 9 10 11 12 13 14 15
//   parity  - 0 1 0 0 1 0 0 1 0  1  1  0  0  1  0
// A child is written with its entries 1 and 2 exchanged iff  parity[mask] XOR swapped XOR (the parent is negatively oriented), so every child
// is positively oriented (((b-a) x (c-a)) . (d-a) >= 0 up to the rounding of its cut vertices).  The parent's orientation is the sign of the
// float32 determinant of the lattice tet -- a lattice tet is never a sliver; a determinant of 0 counts as positive.
#include "d3h_common.h"

#define D3H_TETFILL_ERR_NAN 1

namespace {

constexpr int TF_BLK = 256;

// q of the header comment, two bits per entry, entry 0 lowest
__constant__ uint8_t c_tf_perm[16] = {0xE4, 0xE4, 0xE1, 0xE4, 0xD2, 0xD8, 0xC9, 0xE4, 0x93, 0x9C, 0x8D, 0xB4, 0x4E, 0x78, 0x39, 0xE4};
constexpr unsigned TF_PARITY = 0x4D24u;             // bit m = parity[m]
__constant__ int8_t c_tf_children[5] = {0, 1, 3, 3, 1};

// ordered rank of `flag` inside a 256-thread block (4 waves) and the block total; every thread of the block calls it (as block_rank of
// marching_tets.hip)
__device__ __forceinline__ int tf_block_rank(bool flag, int* s_wave /*[4]*/, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long m = __ballot(flag);
    int r = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) s_wave[wave] = __popcll(m);
    __syncthreads();
    int base = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        int c = s_wave[w];
        if (w < wave) base += c;
        total += c;
    }
    __syncthreads();
    return base + r;
}

__device__ __forceinline__ int tf_inside_mask(const float* __restrict__ sdf, int4 v) {
    return (sdf[v.x] > 0.f ? 0 : 1) | (sdf[v.y] > 0.f ? 0 : 2) | (sdf[v.z] > 0.f ? 0 : 4) | (sdf[v.w] > 0.f ? 0 : 8);
}

// ---- per-workgroup counts: inside vertices, sign-changing edges, children (thread i looks at vertex i, edge i and tet i) -----------------
__global__ __launch_bounds__(TF_BLK) void tf_count(const float* __restrict__ sdf, int nv, const int* __restrict__ tets, int nt,
                                                   const int* __restrict__ edges, int ne, int nbv, int nbe, int nbt, int* __restrict__ blk_v,
                                                   int* __restrict__ blk_e, int* __restrict__ blk_t, int* __restrict__ err) {
    __shared__ int s_wave[4];
    const long long i = (long long)blockIdx.x * TF_BLK + threadIdx.x;
    bool in = false, cross = false;
    int nchild = 0;
    if (i < nv) {
        const float s = sdf[i];
        if (s != s) atomicOr(err, D3H_TETFILL_ERR_NAN);
        in = !(s > 0.f);
    }
    if (i < ne) {
        int2 ab = *(const int2*)(edges + 2 * (size_t)i);
        cross = (sdf[ab.x] > 0.f) != (sdf[ab.y] > 0.f);
    }
    if (i < nt) nchild = c_tf_children[__popc((unsigned)tf_inside_mask(sdf, *(const int4*)(tets + 4 * (size_t)i)))];
    int tv, te, t1, t3;
    tf_block_rank(in, s_wave, tv);
    tf_block_rank(cross, s_wave, te);
    tf_block_rank(nchild == 1, s_wave, t1);
    tf_block_rank(nchild == 3, s_wave, t3);
    if (threadIdx.x == 0) {
        if ((int)blockIdx.x < nbv) blk_v[blockIdx.x] = tv;
        if ((int)blockIdx.x < nbe) blk_e[blockIdx.x] = te;
        if ((int)blockIdx.x < nbt) blk_t[blockIdx.x] = t1 + 3 * t3;
    }
}

// ---- vertices: inside lattice vertices, then the cut vertices (thread i looks at vertex i and edge i) ------------------------------------
__global__ __launch_bounds__(TF_BLK) void tf_emit_verts(const float* __restrict__ pos, const float* __restrict__ sdf, int nv,
                                                        const int* __restrict__ edges, int ne, int nbv, int nbe, const int* __restrict__ off_v,
                                                        const int* __restrict__ off_e, int n_inside, int* __restrict__ vert_id,
                                                        int* __restrict__ edge_vid, float* __restrict__ out_v) {
    __shared__ int s_wave[4];
    const long long i = (long long)blockIdx.x * TF_BLK + threadIdx.x;
    bool in = false, cross = false;
    int2 ab = make_int2(0, 0);
    float s0 = 0.f, s1 = 0.f;
    if (i < nv) in = !(sdf[i] > 0.f);
    if (i < ne) {
        ab = *(const int2*)(edges + 2 * (size_t)i);
        s0 = sdf[ab.x];
        s1 = sdf[ab.y];
        cross = (s0 > 0.f) != (s1 > 0.f);
    }
    int total;
    const int rv = tf_block_rank(in, s_wave, total);
    const int re = tf_block_rank(cross, s_wave, total);
    if (i < nv) {
        const int id = in ? off_v[blockIdx.x] + rv : -1;          // (i < nv: this block is one of the nbv)
        vert_id[i] = id;
        if (in) {
#pragma unroll
            for (int c = 0; c < 3; ++c) out_v[3 * (size_t)id + c] = pos[3 * (size_t)i + c];
        }
    }
    if (i < ne) {
        const int id = cross ? n_inside + off_e[blockIdx.x] + re : -1;
        edge_vid[i] = id;
        if (cross) {
            // mt_emit_verts (marching_tets.hip), gshell_tets.py:291-300
            float a = s0, b = -s1;
            float den = __fadd_rn(a, b);
            float sg = (den > 0.f) ? 1.f : ((den < 0.f) ? -1.f : 0.f);
            den = __fmul_rn(sg, __fadd_rn(fabsf(den), 1e-12f));
            if (den == 0.f) den = 1e-12f;
            float w0 = b / den, w1 = a / den;
#pragma unroll
            for (int c = 0; c < 3; ++c)
                out_v[3 * (size_t)id + c] = __fadd_rn(__fmul_rn(pos[3 * (size_t)ab.x + c], w0), __fmul_rn(pos[3 * (size_t)ab.y + c], w1));
        }
    }
}

// ---- tets ------------------------------------------------------------------------------------------------------------------------
// slot of the edge (a,b) of a tet in the order 01 02 03 12 13 23 of the per-tet edge ids
__device__ __forceinline__ int tf_slot(int a, int b) {
    const int lo = a < b ? a : b, hi = a < b ? b : a;
    return lo == 0 ? hi - 1 : (lo == 1 ? hi + 1 : 5);
}

__device__ __forceinline__ void tf_write(int64_t* __restrict__ out_t, int row, int a, int b, int c, int d, bool flip) {
    int64_t* o = out_t + 4 * (size_t)row;
    o[0] = a;
    o[1] = flip ? c : b;
    o[2] = flip ? b : c;
    o[3] = d;
}

__global__ __launch_bounds__(TF_BLK) void tf_emit_tets(const float* __restrict__ pos, const float* __restrict__ sdf,
                                                       const int* __restrict__ tets, const int* __restrict__ tet_edge, int nt,
                                                       const int* __restrict__ off_t, const int* __restrict__ vert_id,
                                                       const int* __restrict__ edge_vid, int64_t* __restrict__ out_t) {
    __shared__ int s_wave[4];
    const long long t = (long long)blockIdx.x * TF_BLK + threadIdx.x;
    int4 v = make_int4(0, 0, 0, 0);
    int mask = 0, nchild = 0;
    if (t < nt) {
        v = *(const int4*)(tets + 4 * (size_t)t);
        mask = tf_inside_mask(sdf, v);
        nchild = c_tf_children[__popc((unsigned)mask)];
    }
    int total;
    const int r1 = tf_block_rank(nchild == 1, s_wave, total);
    const int r3 = tf_block_rank(nchild == 3, s_wave, total);
    if (nchild == 0) return;
    const int row = off_t[blockIdx.x] + r1 + 3 * r3;
    // orientation of the parent: ((b-a) x (c-a)) . (d-a) in float32
    float e[3][3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float a = pos[3 * (size_t)v.x + c];
        e[0][c] = pos[3 * (size_t)v.y + c] - a;
        e[1][c] = pos[3 * (size_t)v.z + c] - a;
        e[2][c] = pos[3 * (size_t)v.w + c] - a;
    }
    const float det = (e[0][1] * e[1][2] - e[0][2] * e[1][1]) * e[2][0] + (e[0][2] * e[1][0] - e[0][0] * e[1][2]) * e[2][1] +
                      (e[0][0] * e[1][1] - e[0][1] * e[1][0]) * e[2][2];
    bool flip = (((TF_PARITY >> mask) & 1u) != 0) != (det < 0.f);
    const int nin = __popc((unsigned)mask);
    if (nin == 4) {
        tf_write(out_t, row, vert_id[v.x], vert_id[v.y], vert_id[v.z], vert_id[v.w], flip);
        return;
    }
    const int q = c_tf_perm[mask];
    const int q0 = q & 3, q1 = (q >> 2) & 3, q2 = (q >> 4) & 3, q3 = (q >> 6) & 3;
    const int* tv = tets + 4 * (size_t)t;
    const int* te = tet_edge + 6 * (size_t)t;
#define TF_V(k) vert_id[tv[k]]
#define TF_C(i, o) edge_vid[te[tf_slot(i, o)]]
    if (nin == 1) {
        tf_write(out_t, row, TF_V(q0), TF_C(q0, q1), TF_C(q0, q2), TF_C(q0, q3), flip);
        return;
    }
    int p0, p1, p2, p3, p4, p5;
    if (nin == 2) {
        p0 = TF_V(q0); p1 = TF_C(q0, q2); p2 = TF_C(q0, q3);
        p3 = TF_V(q1); p4 = TF_C(q1, q2); p5 = TF_C(q1, q3);
    } else {
        p0 = TF_V(q0); p1 = TF_V(q1); p2 = TF_V(q2);
        p3 = TF_C(q0, q3); p4 = TF_C(q1, q3); p5 = TF_C(q2, q3);
    }
#undef TF_V
#undef TF_C
    const int lo_a = min(p0, min(p1, p2)), lo_b = min(p3, min(p4, p5));
    if (lo_b < lo_a) {                     // the smallest id is in the second triangle: exchange the triangles
        int x;
        x = p0; p0 = p3; p3 = x;
        x = p1; p1 = p4; p4 = x;
        x = p2; p2 = p5; p5 = x;
        flip = !flip;
    }
    const int lo = min(lo_a, lo_b);
    if (p1 == lo) {                        // rotate both triangles together until the smallest id is V0
        int x;
        x = p0; p0 = p1; p1 = p2; p2 = x;
        x = p3; p3 = p4; p4 = p5; p5 = x;
    } else if (p2 == lo) {
        int x;
        x = p0; p0 = p2; p2 = p1; p1 = x;
        x = p3; p3 = p5; p5 = p4; p4 = x;
    }
    if (min(p1, p5) < min(p2, p4)) {
        tf_write(out_t, row + 0, p0, p1, p2, p5, flip);
        tf_write(out_t, row + 1, p0, p1, p5, p4, flip);
        tf_write(out_t, row + 2, p0, p4, p5, p3, flip);
    } else {
        tf_write(out_t, row + 0, p0, p1, p2, p4, flip);
        tf_write(out_t, row + 1, p0, p4, p2, p5, flip);
        tf_write(out_t, row + 2, p0, p4, p5, p3, flip);
    }
}

static inline int tf_nblk(int n) { return n > 0 ? (n + TF_BLK - 1) / TF_BLK : 1; }
static inline int tf_max(int a, int b) { return a > b ? a : b; }

}  // namespace

// ------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------
// per-workgroup counts over 256 items (nb(n) = max(1, ceil(n / 256)) entries each, overwritten): blk_v[nb(nv)] inside vertices (!(sdf > 0)),
// blk_e[nb(ne)] sign-changing edges, blk_t[nb(nt)] children (0, 1, 3, 3, 1 for 0..4 inside corners); a NaN in sdf sets bit 1 of err[0]
// (zeroed by the caller).  tets [nt][4] and edges [ne][2] index sdf [nv]; nt < 2^29
extern "C" int d3h_tetfill_count(const float* sdf, int nv, const int* tets, int nt, const int* edges, int ne, int* blk_v, int* blk_e,
                                 int* blk_t, int* err, void* stream) {
    if (nv < 0 || ne < 0 || nt < 0 || nt >= (1 << 29) || (nv && !sdf) || (nt && !tets) || (ne && !edges) || !blk_v || !blk_e || !blk_t || !err)
        return D3H_ERR_ARG;          // (an empty array may be a null pointer)
    const int nbv = tf_nblk(nv), nbe = tf_nblk(ne), nbt = tf_nblk(nt);
    hipLaunchKernelGGL(tf_count, dim3(tf_max(nbv, tf_max(nbe, nbt))), dim3(TF_BLK), 0, (hipStream_t)stream, sdf, nv, tets, nt, edges, ne, nbv,
                       nbe, nbt, blk_v, blk_e, blk_t, err);
    D3H_LAUNCH_CHECK();
    return D3H_OK;
}

// off_v / off_e: the exclusive scans of blk_v / blk_e; n_inside: the total of blk_v.  Overwritten: vert_id [nv] (new id of an inside
// vertex, else -1), edge_vid [ne] (id of the cut vertex of a sign-changing edge, else -1), out_v [n_inside + total of blk_e][3]: the inside
// vertices in lattice order, then the cut vertices in edge order (the bits of d3h_mtets_emit_wt's verts_wt)
extern "C" int d3h_tetfill_emit_verts(const float* pos, const float* sdf, int nv, const int* edges, int ne, const int* off_v,
                                      const int* off_e, int n_inside, int* vert_id, int* edge_vid, float* out_v, void* stream) {
    if (nv < 0 || ne < 0 || n_inside < 0 || n_inside > nv || (nv && (!pos || !sdf || !vert_id)) || (ne && (!edges || !edge_vid)) || !off_v ||
        !off_e || ((n_inside || ne) && !out_v))
        return D3H_ERR_ARG;
    const int nbv = tf_nblk(nv), nbe = tf_nblk(ne);
    hipLaunchKernelGGL(tf_emit_verts, dim3(tf_max(nbv, nbe)), dim3(TF_BLK), 0, (hipStream_t)stream, pos, sdf, nv, edges, ne, nbv, nbe, off_v,
                       off_e, n_inside, vert_id, edge_vid, out_v);
    D3H_LAUNCH_CHECK();
    return D3H_OK;
}

// off_t: the exclusive scan of blk_t; tet_edge [nt][6]: the edge ids of a tet's corner pairs 01 02 03 12 13 23; vert_id / edge_vid as written
// by d3h_tetfill_emit_verts.  Overwritten: out_t [total of blk_t][4] int64, children in parent order, positively oriented
extern "C" int d3h_tetfill_emit_tets(const float* pos, const float* sdf, const int* tets, const int* tet_edge, int nt, const int* off_t,
                                     const int* vert_id, const int* edge_vid, int64_t* out_t, void* stream) {
    if (nt < 0 || nt >= (1 << 29) || (nt && (!pos || !sdf || !tets || !tet_edge || !vert_id || !out_t)) || !off_t) return D3H_ERR_ARG;
    hipLaunchKernelGGL(tf_emit_tets, dim3(tf_nblk(nt)), dim3(TF_BLK), 0, (hipStream_t)stream, pos, sdf, tets, tet_edge, nt, off_t, vert_id,
                       edge_vid, out_t);
    D3H_LAUNCH_CHECK();
    return D3H_OK;
}
