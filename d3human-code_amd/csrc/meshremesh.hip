// meshremesh.hip -- the collapse, flip and smoothing steps of isotropic remeshing for the stage hand-off, gfx950.
//
// Replaces (reference file:line):
//   script/process_body_cloth_head_msdfcut.py:621,625,661,715  meshlabserver with checkpoints/script/remesh.mlx ("Isotropic Explicit Remeshing":
//   collapse, edge swap, smooth; the refine step is meshrefine.hip, the reprojection is Bvh.nearest of bvhdist.hip)
//
// The host (d3h/meshrefine.py) hands every kernel the adjacency of the mesh as it stands at the start of a round:
//   elo / ehi / ecnt [E]   the unique (min, max) edges in ascending order of (min << 32 | max) with the number of face sides on each; an edge's
//                          RANK is its position
//   noffs [nv+1] / nbr     vertex -> neighbours, ascending per vertex (the ends of the edges with min != max)
//   foffs [nv+1] / vf      vertex -> faces, ascending per vertex
//   pinned [nv]            1 = the vertex lies on an edge that is not used by exactly two face sides, or the caller pinned it
// One thread per edge or per vertex; rows are walked from global memory (no private array, no scratch).  Selection is by a 64-bit atomicMin on one
// claim word per vertex: the minimum does not depend on the arrival order and the selected operations touch disjoint data, so every output is
// bit-reproducible.  No loop can spin: a claim is one atomicMin, every other loop runs over a CSR row.
//
// Arithmetic, float32, every operation rounded once in the order written (contraction off):
//   len2(a, b)   d = b - a;  (dx dx + dy dy) + dz dz
//   dot(u, w)    (ux wx + uy wy) + uz wz
//   cross(u, w)  (uy wz - uz wy,  uz wx - ux wz,  ux wy - uy wx)
//   nrm(p0, p1, p2) = cross(p1 - p0, p2 - p0)
//   cos(n, m) >= c  :=  d = dot(n, m);  d > 0  &&  d d >= c2 (dot(n, n) dot(m, m))       with c2 = c^2 given as a constant (0.25f, 0.75f)
// The rules of the three steps are stated in full in d3h/meshrefine.py; the kernels' comments name the rule they carry out.
#include "d3h_common.h"

#define D3H_TOPO_ERR_RANGE 1

namespace {

constexpr int RM_T = 256;
constexpr unsigned long long RM_FREE = ~0ull;

struct V3 {
    float x, y, z;
};

__device__ __forceinline__ int64_t rm_index(const void* __restrict__ faces, int idx64, int64_t i) {
    return idx64 ? ((const int64_t*)faces)[i] : (int64_t)((const int*)faces)[i];
}

__device__ __forceinline__ void rm_store(void* faces, int idx64, int64_t i, int64_t val) {
    if (idx64) ((int64_t*)faces)[i] = val; else ((int*)faces)[i] = (int)val;
}

__device__ __forceinline__ V3 rm_ld(const float* __restrict__ v, int64_t i) { return V3{v[3 * i], v[3 * i + 1], v[3 * i + 2]}; }

__device__ __forceinline__ V3 rm_sub(V3 a, V3 b) {
#pragma clang fp contract(off)
    return V3{a.x - b.x, a.y - b.y, a.z - b.z};
}

__device__ __forceinline__ float rm_dot(V3 a, V3 b) {
#pragma clang fp contract(off)
    return (a.x * b.x + a.y * b.y) + a.z * b.z;
}

__device__ __forceinline__ float rm_len2(V3 a, V3 b) {
    const V3 d = rm_sub(b, a);
    return rm_dot(d, d);
}

__device__ __forceinline__ V3 rm_cross(V3 u, V3 w) {
#pragma clang fp contract(off)
    return V3{u.y * w.z - u.z * w.y, u.z * w.x - u.x * w.z, u.x * w.y - u.y * w.x};
}

__device__ __forceinline__ V3 rm_nrm(V3 p0, V3 p1, V3 p2) { return rm_cross(rm_sub(p1, p0), rm_sub(p2, p0)); }

__device__ __forceinline__ bool rm_cos(V3 n, V3 m, float c2) {
#pragma clang fp contract(off)
    const float d = rm_dot(n, m);
    return d > 0.f && d * d >= c2 * (rm_dot(n, n) * rm_dot(m, m));
}

// the CSR row of vertex i, clamped to the arrays the host gave: a row that is no row of this mesh is empty
__device__ __forceinline__ void rm_row(const int* __restrict__ offs, int i, int total, int& k0, int& k1) {
    k0 = offs[i], k1 = offs[i + 1];
    if (k0 < 0 || k1 > total || k1 < k0) k0 = k1 = 0;
}

// ---- collapse ------------------------------------------------------------------------------------------------------------------------------

// does the candidate with `key` hold the claim word of every vertex of row i?
__device__ __forceinline__ bool rm_holds_row(const unsigned long long* __restrict__ claim, const int* __restrict__ offs, const int* __restrict__ nbr, int i,
                                             int nnbr, int nv, unsigned long long key) {
    int k0, k1;
    rm_row(offs, i, nnbr, k0, k1);
    for (int k = k0; k < k1; ++k) {
        const int j = nbr[k];
        if (j < 0 || j >= nv || claim[j] != key) return false;
    }
    return true;
}

// every neighbour x of row i but `skip` within hi of q?
__device__ __forceinline__ bool rm_row_within(const float* __restrict__ v, const int* __restrict__ offs, const int* __restrict__ nbr, int i, int skip, int nnbr,
                                              int nv, V3 q, float hi2) {
    int k0, k1;
    rm_row(offs, i, nnbr, k0, k1);
    for (int k = k0; k < k1; ++k) {
        const int x = nbr[k];
        if (x == skip) continue;
        if (x < 0 || x >= nv || !(rm_len2(q, rm_ld(v, x)) <= hi2)) return false;
    }
    return true;
}

// every face of vertex i that does not hold `other` keeps its normal within 60 degrees when i moves to q?
__device__ __forceinline__ bool rm_faces_keep_normal(const float* __restrict__ v, const void* __restrict__ faces, int idx64, int64_t nf, int nv,
                                                     const int* __restrict__ foffs, const int* __restrict__ vf, int nvf, int i, int other, V3 q) {
    int k0, k1;
    rm_row(foffs, i, nvf, k0, k1);
    for (int k = k0; k < k1; ++k) {
        const int f = vf[k];
        if (f < 0 || f >= nf) return false;
        const int64_t i0 = rm_index(faces, idx64, 3 * (int64_t)f), i1 = rm_index(faces, idx64, 3 * (int64_t)f + 1), i2 = rm_index(faces, idx64, 3 * (int64_t)f + 2);
        if (i0 < 0 || i0 >= nv || i1 < 0 || i1 >= nv || i2 < 0 || i2 >= nv) return false;
        if (i0 == other || i1 == other || i2 == other) continue;
        const V3 p0 = rm_ld(v, i0), p1 = rm_ld(v, i1), p2 = rm_ld(v, i2);
        const V3 m = rm_nrm(i0 == i ? q : p0, i1 == i ? q : p1, i2 == i ? q : p2);
        if (!rm_cos(rm_nrm(p0, p1, p2), m, 0.25f)) return false;
    }
    return true;
}

// the new position of a collapse of (a, b): the pinned end's, else the midpoint
__device__ __forceinline__ V3 rm_collapse_point(V3 A, V3 B, bool pa, bool pb) {
#pragma clang fp contract(off)
    return pa ? A : (pb ? B : V3{(A.x + B.x) * 0.5f, (A.y + B.y) * 0.5f, (A.z + B.z) * 0.5f});
}

// one thread per edge: candidate test (face count 2, ends differ, not both pinned, shorter than lo, and the link, length and normal checks, all on
// the round's input), key = bits(len2) << 32 | rank, and the claims on {a, b} + N(a) + N(b)
__global__ __launch_bounds__(RM_T) void collapse_claim_kernel(const float* __restrict__ v, const void* __restrict__ faces, int idx64, int64_t nf, int nv,
                                                              const int* __restrict__ elo, const int* __restrict__ ehi, const int* __restrict__ ecnt, int ne,
                                                              const int* __restrict__ noffs, const int* __restrict__ nbr, int nnbr,
                                                              const int* __restrict__ foffs, const int* __restrict__ vf, int nvf,
                                                              const unsigned char* __restrict__ pinned, float lo, float hi,
                                                              unsigned long long* __restrict__ ekey, unsigned long long* claim, int* counts) {
    const int r = blockIdx.x * RM_T + threadIdx.x;
    if (r >= ne) return;
    const int a = elo[r], b = ehi[r];
    unsigned long long key = RM_FREE;
    if (a < 0 || b < 0 || a >= nv || b >= nv) {
        atomicOr(counts + 2, D3H_TOPO_ERR_RANGE);
    } else if (ecnt[r] == 2 && a != b && !(pinned[a] && pinned[b])) {
#pragma clang fp contract(off)
        const V3 A = rm_ld(v, a), B = rm_ld(v, b);
        const float l2 = rm_len2(A, B);
        bool ok = l2 < lo * lo;
        if (ok) {                                                                // link: exactly two common neighbours, each of valence > 3
            int ia, ia1, ib, ib1, common = 0;
            rm_row(noffs, a, nnbr, ia, ia1);
            rm_row(noffs, b, nnbr, ib, ib1);
            while (ia < ia1 && ib < ib1) {
                const int x = nbr[ia], y = nbr[ib];
                if (x == y) {
                    ++common;
                    if (x < 0 || x >= nv || noffs[x + 1] - noffs[x] <= 3) ok = false;
                    ++ia, ++ib;
                } else if (x < y) {
                    ++ia;
                } else {
                    ++ib;
                }
            }
            ok = ok && common == 2;
        }
        if (ok) {
            const V3 q = rm_collapse_point(A, B, pinned[a] != 0, pinned[b] != 0);
            const float hi2 = hi * hi;
            ok = rm_row_within(v, noffs, nbr, a, b, nnbr, nv, q, hi2) && rm_row_within(v, noffs, nbr, b, a, nnbr, nv, q, hi2) &&
                 rm_faces_keep_normal(v, faces, idx64, nf, nv, foffs, vf, nvf, a, b, q) && rm_faces_keep_normal(v, faces, idx64, nf, nv, foffs, vf, nvf, b, a, q);
        }
        if (ok) key = ((unsigned long long)__float_as_uint(l2) << 32) | (unsigned long long)(unsigned)r;
    }
    ekey[r] = key;
    if (key == RM_FREE) return;
    atomicMin(claim + a, key);
    atomicMin(claim + b, key);
    int k0, k1;
    rm_row(noffs, a, nnbr, k0, k1);
    for (int k = k0; k < k1; ++k) {
        const int j = nbr[k];
        if (j >= 0 && j < nv) atomicMin(claim + j, key);
    }
    rm_row(noffs, b, nnbr, k0, k1);
    for (int k = k0; k < k1; ++k) {
        const int j = nbr[k];
        if (j >= 0 && j < nv) atomicMin(claim + j, key);
    }
}

// one thread per edge: a candidate that holds every claim word of its closed neighbourhood collapses.  Reads v and faces, writes vout (the caller's
// copy of v), remap, fdrop: selected edges have disjoint closed neighbourhoods, so no thread reads what another writes.
__global__ __launch_bounds__(RM_T) void collapse_select_kernel(const float* __restrict__ v, const void* __restrict__ faces, int idx64, int64_t nf, int nv,
                                                               const int* __restrict__ elo, const int* __restrict__ ehi, int ne,
                                                               const int* __restrict__ noffs, const int* __restrict__ nbr, int nnbr,
                                                               const int* __restrict__ foffs, const int* __restrict__ vf, int nvf,
                                                               const unsigned char* __restrict__ pinned,
                                                               const unsigned long long* __restrict__ ekey, const unsigned long long* __restrict__ claim,
                                                               float* __restrict__ vout, int* __restrict__ remap, unsigned char* __restrict__ fdrop,
                                                               int* counts) {
    const int r = blockIdx.x * RM_T + threadIdx.x;
    if (r >= ne) return;
    const unsigned long long key = ekey[r];
    if (key == RM_FREE) return;
    const int a = elo[r], b = ehi[r];
    if (a < 0 || b < 0 || a >= nv || b >= nv) return;
    if (claim[a] != key || claim[b] != key) return;
    if (!rm_holds_row(claim, noffs, nbr, a, nnbr, nv, key) || !rm_holds_row(claim, noffs, nbr, b, nnbr, nv, key)) return;
    const bool pa = pinned[a] != 0, pb = pinned[b] != 0;
    const V3 q = rm_collapse_point(rm_ld(v, a), rm_ld(v, b), pa, pb);
    const int s = pb ? b : a, o = pb ? a : b;                     // (both pinned is no candidate; a is the smaller index)
    vout[3 * (int64_t)s] = q.x, vout[3 * (int64_t)s + 1] = q.y, vout[3 * (int64_t)s + 2] = q.z;
    remap[o] = s;
    int k0, k1, dropped = 0;
    rm_row(foffs, a, nvf, k0, k1);
    for (int k = k0; k < k1; ++k) {
        const int f = vf[k];
        if (f < 0 || f >= nf) continue;
        const int64_t i0 = rm_index(faces, idx64, 3 * (int64_t)f), i1 = rm_index(faces, idx64, 3 * (int64_t)f + 1), i2 = rm_index(faces, idx64, 3 * (int64_t)f + 2);
        if (i0 == b || i1 == b || i2 == b) fdrop[f] = 1, ++dropped;
    }
    atomicAdd(counts, 1);
    atomicAdd(counts + 1, dropped);
}

// one thread per face: a kept face goes to row offs[f] with its indices remapped (removed vertex -> survivor -> new numbering)
__global__ __launch_bounds__(RM_T) void collapse_faces_kernel(const void* __restrict__ faces, int idx64, int64_t nf, int nv, const int* __restrict__ remap,
                                                              const int* __restrict__ newidx, const unsigned char* __restrict__ fdrop,
                                                              const int64_t* __restrict__ offs, int64_t nout, void* __restrict__ out, int* __restrict__ parent) {
    const int64_t f = (int64_t)blockIdx.x * RM_T + threadIdx.x;
    if (f >= nf || fdrop[f]) return;
    const int64_t at = offs[f];
    if (at < 0 || at >= nout) return;                                            // not a scan of these marks: write nothing
    for (int k = 0; k < 3; ++k) {
        const int64_t i = rm_index(faces, idx64, 3 * f + k);
        int64_t j = i;
        if (i >= 0 && i < nv) {
            const int s = remap[i];
            j = (s >= 0 && s < nv) ? newidx[s] : i;
        }
        rm_store(out, idx64, 3 * at + k, j);
    }
    parent[at] = (int)f;
}

// ---- flip ----------------------------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ int rm_absdiff(int a, int b) { return a > b ? a - b : b - a; }

// one thread per edge (a, b) = (min, max): the face that holds a -> b gives c, the face that holds b -> a gives d; candidate test, key =
// (15 - min(gain, 15)) << 32 | rank, claims on a, b, c, d.  equad [E,4] = c, d, face of a -> b, face of b -> a for the apply launch.
__global__ __launch_bounds__(RM_T) void flip_claim_kernel(const float* __restrict__ v, const void* __restrict__ faces, int idx64, int64_t nf, int nv,
                                                          const int* __restrict__ elo, const int* __restrict__ ehi, const int* __restrict__ ecnt, int ne,
                                                          const int* __restrict__ noffs, const int* __restrict__ nbr, int nnbr,
                                                          const int* __restrict__ foffs, const int* __restrict__ vf, int nvf,
                                                          const unsigned char* __restrict__ pinned, unsigned long long* __restrict__ ekey,
                                                          int* __restrict__ equad, unsigned long long* claim, int* counts) {
    const int r = blockIdx.x * RM_T + threadIdx.x;
    if (r >= ne) return;
    const int a = elo[r], b = ehi[r];
    unsigned long long key = RM_FREE;
    int c = -1, d = -1, fab = -1, fba = -1;
    if (a < 0 || b < 0 || a >= nv || b >= nv) {
        atomicOr(counts + 2, D3H_TOPO_ERR_RANGE);
    } else if (ecnt[r] == 2 && a != b) {
        int nab = 0, nba = 0, k0, k1;
        rm_row(foffs, a, nvf, k0, k1);
        for (int k = k0; k < k1; ++k) {
            const int f = vf[k];
            if (f < 0 || f >= nf) continue;
            const int64_t i0 = rm_index(faces, idx64, 3 * (int64_t)f), i1 = rm_index(faces, idx64, 3 * (int64_t)f + 1), i2 = rm_index(faces, idx64, 3 * (int64_t)f + 2);
            if (i0 < 0 || i0 >= nv || i1 < 0 || i1 >= nv || i2 < 0 || i2 >= nv) continue;
            if (i0 == a && i1 == b) ++nab, fab = f, c = (int)i2;
            if (i1 == a && i2 == b) ++nab, fab = f, c = (int)i0;
            if (i2 == a && i0 == b) ++nab, fab = f, c = (int)i1;
            if (i0 == b && i1 == a) ++nba, fba = f, d = (int)i2;
            if (i1 == b && i2 == a) ++nba, fba = f, d = (int)i0;
            if (i2 == b && i0 == a) ++nba, fba = f, d = (int)i1;
        }
        bool cand = nab == 1 && nba == 1 && fab != fba && c != d && c != a && c != b && d != a && d != b;
        if (cand) {                                                              // the edge (c, d) must not exist
            rm_row(noffs, c, nnbr, k0, k1);
            for (int k = k0; k < k1; ++k) cand = cand && nbr[k] != d;
        }
        int gain = 0;
        if (cand) {
            const int va = noffs[a + 1] - noffs[a], vb = noffs[b + 1] - noffs[b], vc = noffs[c + 1] - noffs[c], vd = noffs[d + 1] - noffs[d];
            const int ta = pinned[a] ? 4 : 6, tb = pinned[b] ? 4 : 6, tc = pinned[c] ? 4 : 6, td = pinned[d] ? 4 : 6;
            gain = (rm_absdiff(va, ta) + rm_absdiff(vb, tb) + rm_absdiff(vc, tc) + rm_absdiff(vd, td)) -
                   (rm_absdiff(va - 1, ta) + rm_absdiff(vb - 1, tb) + rm_absdiff(vc + 1, tc) + rm_absdiff(vd + 1, td));
            cand = gain > 0;
        }
        if (cand) {
            const V3 A = rm_ld(v, a), B = rm_ld(v, b), C = rm_ld(v, c), D = rm_ld(v, d);
            const V3 n1 = rm_nrm(A, B, C), n2 = rm_nrm(B, A, D);                // the old faces, rotated to (a, b, c) and (b, a, d)
            const V3 m1 = rm_nrm(A, D, C), m2 = rm_nrm(D, B, C);                // the new faces (a, d, c) and (d, b, c)
            cand = rm_cos(n1, n2, 0.75f) && rm_cos(m1, n1, 0.25f) && rm_cos(m1, n2, 0.25f) && rm_cos(m2, n1, 0.25f) && rm_cos(m2, n2, 0.25f);
        }
        if (cand) key = ((unsigned long long)(15 - (gain < 15 ? gain : 15)) << 32) | (unsigned long long)(unsigned)r;
    }
    ekey[r] = key;
    equad[4 * (int64_t)r] = c, equad[4 * (int64_t)r + 1] = d, equad[4 * (int64_t)r + 2] = fab, equad[4 * (int64_t)r + 3] = fba;
    if (key == RM_FREE) return;
    atomicMin(claim + a, key);
    atomicMin(claim + b, key);
    atomicMin(claim + c, key);
    atomicMin(claim + d, key);
}

// one thread per edge: a candidate that holds a, b, c and d flips in place.  Reads only what the claim launch wrote, so a face another thread
// rewrites is never read; selected edges have disjoint vertex sets, hence disjoint faces.
__global__ __launch_bounds__(RM_T) void flip_apply_kernel(void* faces, int idx64, int64_t nf, int nv, const int* __restrict__ elo, const int* __restrict__ ehi,
                                                          int ne, const unsigned long long* __restrict__ ekey, const int* __restrict__ equad,
                                                          const unsigned long long* __restrict__ claim, int* counts) {
    const int r = blockIdx.x * RM_T + threadIdx.x;
    if (r >= ne) return;
    const unsigned long long key = ekey[r];
    if (key == RM_FREE) return;
    const int a = elo[r], b = ehi[r], c = equad[4 * (int64_t)r], d = equad[4 * (int64_t)r + 1];
    const int64_t fab = equad[4 * (int64_t)r + 2], fba = equad[4 * (int64_t)r + 3];
    if (a < 0 || a >= nv || b < 0 || b >= nv || c < 0 || c >= nv || d < 0 || d >= nv || fab < 0 || fab >= nf || fba < 0 || fba >= nf) return;
    if (claim[a] != key || claim[b] != key || claim[c] != key || claim[d] != key) return;
    rm_store(faces, idx64, 3 * fab, a), rm_store(faces, idx64, 3 * fab + 1, d), rm_store(faces, idx64, 3 * fab + 2, c);
    rm_store(faces, idx64, 3 * fba, d), rm_store(faces, idx64, 3 * fba + 1, b), rm_store(faces, idx64, 3 * fba + 2, c);
    atomicAdd(counts, 1);
}

// ---- tangential smoothing ------------------------------------------------------------------------------------------------------------------

// one thread per vertex, one Jacobi pass: reads v, writes vout
__global__ __launch_bounds__(RM_T) void smooth_kernel(const float* __restrict__ v, const void* __restrict__ faces, int idx64, int64_t nf, int nv,
                                                      const int* __restrict__ noffs, const int* __restrict__ nbr, int nnbr, const int* __restrict__ foffs,
                                                      const int* __restrict__ vf, int nvf, const unsigned char* __restrict__ pinned,
                                                      float* __restrict__ vout) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * RM_T + threadIdx.x;
    if (i >= nv) return;
    const V3 p = rm_ld(v, i);
    V3 o = p;
    int k0, k1, f0, f1;
    rm_row(noffs, i, nnbr, k0, k1);
    rm_row(foffs, i, nvf, f0, f1);
    if (!pinned[i] && k1 > k0) {
        V3 g{0.f, 0.f, 0.f}, n{0.f, 0.f, 0.f};
        bool ok = true;
        for (int k = k0; k < k1; ++k) {
            const int j = nbr[k];
            if (j < 0 || j >= nv) { ok = false; continue; }
            const V3 x = rm_ld(v, j);
            g.x += x.x, g.y += x.y, g.z += x.z;
        }
        const float inv = 1.0f / (float)(k1 - k0);
        g.x *= inv, g.y *= inv, g.z *= inv;
        for (int k = f0; k < f1; ++k) {
            const int f = vf[k];
            if (f < 0 || f >= nf) { ok = false; continue; }
            const int64_t i0 = rm_index(faces, idx64, 3 * (int64_t)f), i1 = rm_index(faces, idx64, 3 * (int64_t)f + 1), i2 = rm_index(faces, idx64, 3 * (int64_t)f + 2);
            if (i0 < 0 || i0 >= nv || i1 < 0 || i1 >= nv || i2 < 0 || i2 >= nv) { ok = false; continue; }
            const V3 m = rm_nrm(rm_ld(v, i0), rm_ld(v, i1), rm_ld(v, i2));
            n.x += m.x, n.y += m.y, n.z += m.z;
        }
        const float nn = rm_dot(n, n);
        if (ok && nn > 0.f) {
            const float len = sqrtf(nn);
            n.x /= len, n.y /= len, n.z /= len;
            const V3 d = rm_sub(g, p);
            const float t = rm_dot(n, d);
            const V3 q{(p.x + d.x) - n.x * t, (p.y + d.y) - n.y * t, (p.z + d.z) - n.z * t};
            for (int k = f0; k < f1; ++k) {                                      // rejected when a face of the vertex would turn over
                const int f = vf[k];
                const int64_t i0 = rm_index(faces, idx64, 3 * (int64_t)f), i1 = rm_index(faces, idx64, 3 * (int64_t)f + 1), i2 = rm_index(faces, idx64, 3 * (int64_t)f + 2);
                const V3 p0 = rm_ld(v, i0), p1 = rm_ld(v, i1), p2 = rm_ld(v, i2);
                const V3 m = rm_nrm(i0 == i ? q : p0, i1 == i ? q : p1, i2 == i ? q : p2);
                if (!(rm_dot(m, rm_nrm(p0, p1, p2)) > 0.f)) ok = false;
            }
            if (ok) o = q;
        }
    }
    vout[3 * (int64_t)i] = o.x, vout[3 * (int64_t)i + 1] = o.y, vout[3 * (int64_t)i + 2] = o.z;
}

inline bool rm_misaligned(const void* p, size_t a) { return ((uintptr_t)p & (a - 1)) != 0; }
inline unsigned rm_blocks(int64_t n) { return (unsigned)((n + RM_T - 1) / RM_T); }
inline bool rm_bad_sizes(int64_t nf, int nv, int ne, int nnbr, int nvf) {
    return nf < 0 || nf > 0x7fffffff / 3 || nv < 0 || ne < 0 || nnbr < 0 || nvf < 0;
}

}  // namespace

// Collapse round, first launch.  v [nv,3] float32; faces [nf,3] int32 (idx64 = 0) or int64 (1); elo / ehi / ecnt [ne] int32: the unique (min, max) edges,
// ascending in (min << 32 | max), and the face sides on each; noffs [nv+1] / nbr [nnbr] int32: vertex -> neighbours CSR, ascending per vertex; foffs
// [nv+1] / vf [nvf] int32: vertex -> faces CSR, ascending per vertex; pinned [nv] uint8; lo: the collapse length; hi: no edge longer than hi may come
// out of a collapse.  ekey [ne] uint64 overwritten: bits(len2) << 32 | rank of a candidate (face count 2, min != max, not both ends pinned,
// len2 < lo lo, link / length / normal checks passed), all ones otherwise; claim [nv] uint64 overwritten: the smallest key among the candidates
// whose closed neighbourhood {a, b} + N(a) + N(b) holds the vertex; counts [4] int32, accumulated: word 2 is the error word (bit 1 = an index
// out of range).
extern "C" int d3h_remesh_collapse_claim(const float* v, const void* faces, int idx64, int64_t nf, int nv, const int* elo, const int* ehi, const int* ecnt, int ne,
                                         const int* noffs, const int* nbr, int nnbr, const int* foffs, const int* vf, int nvf, const unsigned char* pinned, float lo,
                                         float hi, unsigned long long* ekey, unsigned long long* claim, int* counts, void* stream) {
    if (rm_bad_sizes(nf, nv, ne, nnbr, nvf) || !(lo >= 0.f) || !(hi >= 0.f)) return D3H_ERR_ARG;
    if (nv == 0 || ne == 0 || nf == 0) return D3H_OK;
    if (!v || !faces || !elo || !ehi || !ecnt || !noffs || (nnbr > 0 && !nbr) || !foffs || (nvf > 0 && !vf) || !pinned || !ekey || !claim || !counts ||
        rm_misaligned(faces, idx64 ? 8 : 4) || rm_misaligned(ekey, 8) || rm_misaligned(claim, 8))
        return D3H_ERR_ARG;
    const hipError_t e = hipMemsetAsync(claim, 0xff, sizeof(unsigned long long) * (size_t)nv, (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(collapse_claim_kernel, dim3(rm_blocks(ne)), dim3(RM_T), 0, (hipStream_t)stream, v, faces, idx64, nf, nv, elo, ehi, ecnt, ne, noffs, nbr, nnbr,
                       foffs, vf, nvf, pinned, lo, hi, ekey, claim, counts);
    D3H_LAUNCH_CHECK();
    return D3H_OK;
}

// Collapse round, second launch (arrays as in the first; ekey / claim: its outputs).  A candidate that holds the claim word of its whole closed
// neighbourhood collapses: vout [nv,3] (the caller's copy of v) gets the new position in the survivor's row, remap [nv] int32 (the caller's
// identity) gets the survivor in the removed vertex's row, fdrop [nf] uint8 (the caller's zeros) gets 1 for the two faces that held both ends;
// counts [4] int32, accumulated: collapses, dropped faces, error word.
extern "C" int d3h_remesh_collapse_select(const float* v, const void* faces, int idx64, int64_t nf, int nv, const int* elo, const int* ehi, int ne,
                                          const int* noffs, const int* nbr, int nnbr, const int* foffs, const int* vf, int nvf, const unsigned char* pinned,
                                          const unsigned long long* ekey, const unsigned long long* claim, float* vout, int* remap, unsigned char* fdrop,
                                          int* counts, void* stream) {
    if (rm_bad_sizes(nf, nv, ne, nnbr, nvf)) return D3H_ERR_ARG;
    if (nv == 0 || ne == 0 || nf == 0) return D3H_OK;
    if (!v || !faces || !elo || !ehi || !noffs || (nnbr > 0 && !nbr) || !foffs || (nvf > 0 && !vf) || !pinned || !ekey || !claim || !vout || v == vout || !remap ||
        !fdrop || !counts || rm_misaligned(faces, idx64 ? 8 : 4) || rm_misaligned(ekey, 8) || rm_misaligned(claim, 8))
        return D3H_ERR_ARG;
    hipLaunchKernelGGL(collapse_select_kernel, dim3(rm_blocks(ne)), dim3(RM_T), 0, (hipStream_t)stream, v, faces, idx64, nf, nv, elo, ehi, ne, noffs, nbr, nnbr, foffs,
                       vf, nvf, pinned, ekey, claim, vout, remap, fdrop, counts);
    D3H_LAUNCH_CHECK();
    return D3H_OK;
}

// Collapse round, third launch.  remap [nv] int32: old vertex -> survivor (itself when it stays); newidx [nv] int32: survivor -> its row once the
// removed vertices are taken out; fdrop [nf] uint8; offs [nf] int64: the exclusive scan of 1 - fdrop; out [nout,3] of the faces' type and parent
// [nout] int32 overwritten: the kept faces in order, indices renumbered, and the input face of each.
extern "C" int d3h_remesh_collapse_faces(const void* faces, int idx64, int64_t nf, int nv, const int* remap, const int* newidx, const unsigned char* fdrop,
                                         const int64_t* offs, int64_t nout, void* out, int* parent, void* stream) {
    if (rm_bad_sizes(nf, nv, 0, 0, 0) || nout < 0 || nout > nf) return D3H_ERR_ARG;
    if (nf == 0) return D3H_OK;
    if (!faces || !remap || !newidx || !fdrop || !offs || (nout > 0 && (!out || !parent)) || rm_misaligned(faces, idx64 ? 8 : 4) ||
        rm_misaligned(out, idx64 ? 8 : 4) || rm_misaligned(offs, 8))
        return D3H_ERR_ARG;
    hipLaunchKernelGGL(collapse_faces_kernel, dim3(rm_blocks(nf)), dim3(RM_T), 0, (hipStream_t)stream, faces, idx64, nf, nv, remap, newidx, fdrop, offs, nout, out,
                       parent);
    D3H_LAUNCH_CHECK();
    return D3H_OK;
}

// Flip round, first launch (arrays as in the collapse launches).  ekey [ne] uint64 overwritten: (15 - min(gain, 15)) << 32 | rank of a candidate, all
// ones otherwise; equad [ne,4] int32 overwritten: c, d, the face that holds min -> max, the face that holds max -> min (-1 where there is none);
// claim [nv] uint64 overwritten: the smallest key among the candidates whose a, b, c, d hold the vertex; counts [4] int32: word 2 the error word.
extern "C" int d3h_remesh_flip_claim(const float* v, const void* faces, int idx64, int64_t nf, int nv, const int* elo, const int* ehi, const int* ecnt, int ne,
                                     const int* noffs, const int* nbr, int nnbr, const int* foffs, const int* vf, int nvf, const unsigned char* pinned,
                                     unsigned long long* ekey, int* equad, unsigned long long* claim, int* counts, void* stream) {
    if (rm_bad_sizes(nf, nv, ne, nnbr, nvf)) return D3H_ERR_ARG;
    if (nv == 0 || ne == 0 || nf == 0) return D3H_OK;
    if (!v || !faces || !elo || !ehi || !ecnt || !noffs || (nnbr > 0 && !nbr) || !foffs || (nvf > 0 && !vf) || !pinned || !ekey || !equad || !claim || !counts ||
        rm_misaligned(faces, idx64 ? 8 : 4) || rm_misaligned(ekey, 8) || rm_misaligned(claim, 8))
        return D3H_ERR_ARG;
    const hipError_t e = hipMemsetAsync(claim, 0xff, sizeof(unsigned long long) * (size_t)nv, (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(flip_claim_kernel, dim3(rm_blocks(ne)), dim3(RM_T), 0, (hipStream_t)stream, v, faces, idx64, nf, nv, elo, ehi, ecnt, ne, noffs, nbr, nnbr, foffs,
                       vf, nvf, pinned, ekey, equad, claim, counts);
    D3H_LAUNCH_CHECK();
    return D3H_OK;
}

// Flip round, second launch.  faces [nf,3] is rewritten in place: for a candidate that holds a, b, c and d the face that held a -> b becomes
// (a, d, c) and the face that held b -> a becomes (d, b, c); counts [4] int32, accumulated: word 0 the number of flips.
extern "C" int d3h_remesh_flip_apply(void* faces, int idx64, int64_t nf, int nv, const int* elo, const int* ehi, int ne, const unsigned long long* ekey,
                                     const int* equad, const unsigned long long* claim, int* counts, void* stream) {
    if (rm_bad_sizes(nf, nv, ne, 0, 0)) return D3H_ERR_ARG;
    if (nv == 0 || ne == 0 || nf == 0) return D3H_OK;
    if (!faces || !elo || !ehi || !ekey || !equad || !claim || !counts || rm_misaligned(faces, idx64 ? 8 : 4) || rm_misaligned(ekey, 8) || rm_misaligned(claim, 8))
        return D3H_ERR_ARG;
    hipLaunchKernelGGL(flip_apply_kernel, dim3(rm_blocks(ne)), dim3(RM_T), 0, (hipStream_t)stream, faces, idx64, nf, nv, elo, ehi, ne, ekey, equad, claim, counts);
    D3H_LAUNCH_CHECK();
    return D3H_OK;
}

// One Jacobi pass of tangential smoothing (arrays as above): vout [nv,3] float32 overwritten, != v.  A vertex that is not pinned and has a neighbour
// moves to p + d - n dot(n, d), d = mean of the neighbours - p, n = the normalised sum of its faces' normals, unless a face of it would turn over;
// every other vertex is copied bit for bit.
extern "C" int d3h_remesh_smooth(const float* v, const void* faces, int idx64, int64_t nf, int nv, const int* noffs, const int* nbr, int nnbr, const int* foffs,
                                 const int* vf, int nvf, const unsigned char* pinned, float* vout, void* stream) {
    if (rm_bad_sizes(nf, nv, 0, nnbr, nvf)) return D3H_ERR_ARG;
    if (nv == 0) return D3H_OK;
    if (!v || !vout || v == vout || !noffs || (nnbr > 0 && !nbr) || !foffs || (nvf > 0 && !vf) || !pinned || (nf > 0 && !faces) ||
        rm_misaligned(faces, idx64 ? 8 : 4))
        return D3H_ERR_ARG;
    hipLaunchKernelGGL(smooth_kernel, dim3(rm_blocks(nv)), dim3(RM_T), 0, (hipStream_t)stream, v, faces, idx64, nf, nv, noffs, nbr, nnbr, foffs, vf, nvf, pinned, vout);
    D3H_LAUNCH_CHECK();
    return D3H_OK;
}
