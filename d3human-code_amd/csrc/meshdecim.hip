// meshdecim.hip -- quadric-error-metric decimation (Garland & Heckbert 1997) in rounds of independent edge collapses, for the level-of-detail
// export (d3h/export.py: lod_chain), gfx950.
//
// No reference counterpart: the reference exports one level of detail (train.py:198-246).  The collapse machinery is that of meshremesh.hip and the
// host (d3h/meshrefine.py: decimate) hands every kernel the same adjacency of the mesh as it stands at the start of a round:
//   elo / ehi / ecnt [E]   the unique (min, max) edges in ascending order of (min << 32 | max) with the number of face sides on each; an edge's
//                          RANK is its position
//   noffs [nv+1] / nbr     vertex -> neighbours, ascending per vertex;  ncnt [nnbr]: the face count of the edge to that neighbour
//   foffs [nv+1] / vf      vertex -> faces, ascending per vertex
//   vclass [nv]            0 = interior, 1 = boundary (on exactly two edges of face count 1), 2 = pinned
//   Q [nv,10]              float64 quadrics (a00, a01, a02, b0, a11, a12, b1, a22, b2, c): E(q) = q^T A q + 2 b^T q + c
// One thread per vertex (quadrics) or per edge (everything else); rows are walked from global memory (no private array, no scratch).  Selection is
// by a 64-bit atomicMin on one claim word per vertex, so every output is bit-reproducible.  No loop can spin: a claim is one atomicMin, every other
// loop runs over a CSR row.  An index out of range sets the error word (counts word 2, bit 1) and is not followed.
//
// Arithmetic: quadrics, placement and cost in float64, the normal test in float32 (the conventions of meshremesh.hip), every operation rounded once
// in the order written (contraction off):
//   dot(u, w)    (ux wx + uy wy) + uz wz                     len2(a, b)  d = b - a; dot(d, d)
//   cross(u, w)  (uy wz - uz wy,  uz wx - ux wz,  ux wy - uy wx)
//   det3(m)      (m00 (m11 m22 - m12 m21) - m01 (m10 m22 - m12 m20)) + m02 (m10 m21 - m11 m20)
//   E(q)         r = ((a00 x + a01 y) + a02 z,  (a01 x + a11 y) + a12 z,  (a02 x + a12 y) + a22 z);
//                e = (((x rx + y ry) + z rz) + 2 ((b0 x + b1 y) + b2 z)) + c;  e < 0 gives 0
// The rules are stated in full in d3h/meshrefine.py; the kernels' comments name the rule they carry out.
#include "d3h_common.h"

#define D3H_TOPO_ERR_RANGE 1

namespace {

constexpr int DC_T = 256;
constexpr unsigned long long DC_FREE = 0x7fffffffffffffffull;      // no key: above every key, and the largest value of the int64 the host sorts
constexpr double DC_BOUNDARY_WEIGHT = 4.0;                            // weight of a boundary edge's plane, times dot(e, e)
constexpr double DC_DET_EPS = 1e-9;                                   // the optimum is taken when |det| > DC_DET_EPS trace^3
constexpr double DC_REACH = 4.0;                                      // ... and it lies within sqrt(DC_REACH) edge lengths of the midpoint
constexpr float DC_COS2 = 0.04f;                                      // normal test: cos >= 0.2

struct F3 {
    float x, y, z;
};
struct D3 {
    double x, y, z;
};
struct Quad {
    double m[10];
};

__device__ __forceinline__ int64_t dc_index(const void* __restrict__ faces, int idx64, int64_t i) {
    return idx64 ? ((const int64_t*)faces)[i] : (int64_t)((const int*)faces)[i];
}

__device__ __forceinline__ F3 dc_ld(const float* __restrict__ v, int64_t i) { return F3{v[3 * i], v[3 * i + 1], v[3 * i + 2]}; }
__device__ __forceinline__ D3 dc_ldd(const float* __restrict__ v, int64_t i) { return D3{(double)v[3 * i], (double)v[3 * i + 1], (double)v[3 * i + 2]}; }
__device__ __forceinline__ D3 dc_wide(F3 p) { return D3{(double)p.x, (double)p.y, (double)p.z}; }

__device__ __forceinline__ F3 dc_sub(F3 a, F3 b) {
#pragma clang fp contract(off)
    return F3{a.x - b.x, a.y - b.y, a.z - b.z};
}
__device__ __forceinline__ float dc_dot(F3 a, F3 b) {
#pragma clang fp contract(off)
    return (a.x * b.x + a.y * b.y) + a.z * b.z;
}
__device__ __forceinline__ F3 dc_cross(F3 u, F3 w) {
#pragma clang fp contract(off)
    return F3{u.y * w.z - u.z * w.y, u.z * w.x - u.x * w.z, u.x * w.y - u.y * w.x};
}
__device__ __forceinline__ F3 dc_nrm(F3 p0, F3 p1, F3 p2) { return dc_cross(dc_sub(p1, p0), dc_sub(p2, p0)); }
__device__ __forceinline__ bool dc_cos(F3 n, F3 m, float c2) {
#pragma clang fp contract(off)
    const float d = dc_dot(n, m);
    return d > 0.f && d * d >= c2 * (dc_dot(n, n) * dc_dot(m, m));
}

__device__ __forceinline__ D3 dc_sub(D3 a, D3 b) {
#pragma clang fp contract(off)
    return D3{a.x - b.x, a.y - b.y, a.z - b.z};
}
__device__ __forceinline__ double dc_dot(D3 a, D3 b) {
#pragma clang fp contract(off)
    return (a.x * b.x + a.y * b.y) + a.z * b.z;
}
__device__ __forceinline__ D3 dc_cross(D3 u, D3 w) {
#pragma clang fp contract(off)
    return D3{u.y * w.z - u.z * w.y, u.z * w.x - u.x * w.z, u.x * w.y - u.y * w.x};
}
__device__ __forceinline__ double dc_len2(D3 a, D3 b) {
    const D3 d = dc_sub(b, a);
    return dc_dot(d, d);
}
__device__ __forceinline__ double dc_det3(double m00, double m01, double m02, double m10, double m11, double m12, double m20, double m21, double m22) {
#pragma clang fp contract(off)
    return (m00 * (m11 * m22 - m12 * m21) - m01 * (m10 * m22 - m12 * m20)) + m02 * (m10 * m21 - m11 * m20);
}

// the CSR row of vertex i, clamped to the arrays the host gave: a row that is no row of this mesh is empty
__device__ __forceinline__ void dc_row(const int* __restrict__ offs, int i, int total, int& k0, int& k1) {
    k0 = offs[i], k1 = offs[i + 1];
    if (k0 < 0 || k1 > total || k1 < k0) k0 = k1 = 0;
}

// Q += w (n n^T, d n, d d) for the plane dot(n, x) + d = 0
__device__ __forceinline__ void dc_add_plane(Quad& Q, D3 n, double d, double w) {
#pragma clang fp contract(off)
    Q.m[0] += w * (n.x * n.x), Q.m[1] += w * (n.x * n.y), Q.m[2] += w * (n.x * n.z), Q.m[3] += w * (n.x * d);
    Q.m[4] += w * (n.y * n.y), Q.m[5] += w * (n.y * n.z), Q.m[6] += w * (n.y * d);
    Q.m[7] += w * (n.z * n.z), Q.m[8] += w * (n.z * d);
    Q.m[9] += w * (d * d);
}

__device__ __forceinline__ double dc_error(const Quad& Q, D3 q) {
#pragma clang fp contract(off)
    const double rx = (Q.m[0] * q.x + Q.m[1] * q.y) + Q.m[2] * q.z;
    const double ry = (Q.m[1] * q.x + Q.m[4] * q.y) + Q.m[5] * q.z;
    const double rz = (Q.m[2] * q.x + Q.m[5] * q.y) + Q.m[7] * q.z;
    const double e = (((q.x * rx + q.y * ry) + q.z * rz) + 2.0 * ((Q.m[3] * q.x + Q.m[6] * q.y) + Q.m[8] * q.z)) + Q.m[9];
    return e < 0.0 ? 0.0 : e;
}

// p replaces q when its error is smaller (a tie keeps the earlier)
__device__ __forceinline__ void dc_try(const Quad& Q, F3 p, double& cost, F3& q) {
    const double e = dc_error(Q, dc_wide(p));
    if (e < cost) cost = e, q = p;
}

// the unit normal of face f and twice its area; false when an index is out of range or the area is 0
__device__ __forceinline__ bool dc_face_plane(const float* __restrict__ v, const void* __restrict__ faces, int idx64, int nv, int64_t f, D3& u, double& l, D3& p0,
                                              int64_t& i0, int64_t& i1, int64_t& i2, bool& range) {
#pragma clang fp contract(off)
    i0 = dc_index(faces, idx64, 3 * f), i1 = dc_index(faces, idx64, 3 * f + 1), i2 = dc_index(faces, idx64, 3 * f + 2);
    if (i0 < 0 || i0 >= nv || i1 < 0 || i1 >= nv || i2 < 0 || i2 >= nv) {
        range = true;
        return false;
    }
    p0 = dc_ldd(v, i0);
    const D3 n = dc_cross(dc_sub(dc_ldd(v, i1), p0), dc_sub(dc_ldd(v, i2), p0));
    l = sqrt(dc_dot(n, n));
    if (!(l > 0.0)) return false;
    u = D3{n.x / l, n.y / l, n.z / l};
    return true;
}

// one thread per vertex: the planes of its faces in ascending face index, then (slide) of its boundary edges in ascending edge rank, which is the
// order of its neighbour row: (j, i) with j < i ranks before (i, j') and both run with j
__global__ __launch_bounds__(DC_T) void decim_quadrics_kernel(const float* __restrict__ v, const void* __restrict__ faces, int idx64, int64_t nf, int nv,
                                                              const int* __restrict__ noffs, const int* __restrict__ nbr, const int* __restrict__ ncnt, int nnbr,
                                                              const int* __restrict__ foffs, const int* __restrict__ vf, int nvf, int slide,
                                                              double* __restrict__ Qout, int* counts) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * DC_T + threadIdx.x;
    if (i >= nv) return;
    Quad Q;
    for (int k = 0; k < 10; ++k) Q.m[k] = 0.0;
    bool range = false;
    int f0, f1;
    dc_row(foffs, i, nvf, f0, f1);
    for (int k = f0; k < f1; ++k) {
        const int f = vf[k];
        if (f < 0 || f >= nf) {
            range = true;
            continue;
        }
        D3 u, p0;
        double l;
        int64_t i0, i1, i2;
        if (!dc_face_plane(v, faces, idx64, nv, f, u, l, p0, i0, i1, i2, range)) continue;
        dc_add_plane(Q, u, -dc_dot(u, p0), l * 0.5);
    }
    if (slide) {
        int k0, k1;
        dc_row(noffs, i, nnbr, k0, k1);
        for (int k = k0; k < k1; ++k) {
            if (ncnt[k] != 1) continue;
            const int j = nbr[k];
            if (j < 0 || j >= nv) {
                range = true;
                continue;
            }
            for (int kk = f0; kk < f1; ++kk) {                                  // the one face of the edge (the first that holds j)
                const int f = vf[kk];
                if (f < 0 || f >= nf) continue;
                if (dc_index(faces, idx64, 3 * (int64_t)f) != j && dc_index(faces, idx64, 3 * (int64_t)f + 1) != j && dc_index(faces, idx64, 3 * (int64_t)f + 2) != j)
                    continue;
                D3 u, p0;
                double l;
                int64_t i0, i1, i2;
                if (dc_face_plane(v, faces, idx64, nv, f, u, l, p0, i0, i1, i2, range)) {
                    const int a = i < j ? i : j, b = i < j ? j : i;
                    const D3 pa = dc_ldd(v, a);
                    const D3 e = dc_sub(dc_ldd(v, b), pa);
                    const D3 m = dc_cross(e, u);
                    const double lm = sqrt(dc_dot(m, m));
                    if (lm > 0.0) {
                        const D3 mu{m.x / lm, m.y / lm, m.z / lm};
                        dc_add_plane(Q, mu, -dc_dot(mu, pa), DC_BOUNDARY_WEIGHT * dc_dot(e, e));
                    }
                }
                break;
            }
        }
    }
    if (range) atomicOr(counts + 2, D3H_TOPO_ERR_RANGE);
    for (int k = 0; k < 10; ++k) Qout[10 * (int64_t)i + k] = Q.m[k];
}

// every face of vertex i that does not hold `other` keeps its normal within acos(0.2) when i moves to q?
__device__ __forceinline__ bool dc_faces_keep_normal(const float* __restrict__ v, const void* __restrict__ faces, int idx64, int64_t nf, int nv,
                                                     const int* __restrict__ foffs, const int* __restrict__ vf, int nvf, int i, int other, F3 q) {
    int k0, k1;
    dc_row(foffs, i, nvf, k0, k1);
    for (int k = k0; k < k1; ++k) {
        const int f = vf[k];
        if (f < 0 || f >= nf) return false;
        const int64_t i0 = dc_index(faces, idx64, 3 * (int64_t)f), i1 = dc_index(faces, idx64, 3 * (int64_t)f + 1), i2 = dc_index(faces, idx64, 3 * (int64_t)f + 2);
        if (i0 < 0 || i0 >= nv || i1 < 0 || i1 >= nv || i2 < 0 || i2 >= nv) return false;
        if (i0 == other || i1 == other || i2 == other) continue;
        const F3 p0 = dc_ld(v, i0), p1 = dc_ld(v, i1), p2 = dc_ld(v, i2);
        const F3 m = dc_nrm(i0 == i ? q : p0, i1 == i ? q : p1, i2 == i ? q : p2);
        if (!dc_cos(dc_nrm(p0, p1, p2), m, DC_COS2)) return false;
    }
    return true;
}

// a stated bijection of 32-bit words: the rank, salted by the round, through the finaliser of MurmurHash3
__device__ __forceinline__ unsigned dc_mix(unsigned rank, unsigned round) {
    unsigned x = rank ^ (round * 0x9e3779b9u);
    x ^= x >> 16;
    x *= 0x85ebca6bu;
    x ^= x >> 13;
    x *= 0xc2b2ae35u;
    x ^= x >> 16;
    return x;
}

// one thread per edge: class, placement, cost and the link and normal checks, all on the round's input
__global__ __launch_bounds__(DC_T) void decim_cost_kernel(const float* __restrict__ v, const void* __restrict__ faces, int idx64, int64_t nf, int nv,
                                                          const int* __restrict__ elo, const int* __restrict__ ehi, const int* __restrict__ ecnt, int ne,
                                                          const int* __restrict__ noffs, const int* __restrict__ nbr, int nnbr,
                                                          const int* __restrict__ foffs, const int* __restrict__ vf, int nvf,
                                                          const unsigned char* __restrict__ vclass, const double* __restrict__ Q, double max_cost, int slide,
                                                          unsigned round, unsigned long long* __restrict__ wkey, unsigned long long* __restrict__ ekey,
                                                          float* __restrict__ eq, int* __restrict__ esurv, double* __restrict__ ecost, int* counts) {
#pragma clang fp contract(off)
    const int r = blockIdx.x * DC_T + threadIdx.x;
    if (r >= ne) return;
    const int a = elo[r], b = ehi[r], cnt = ecnt[r];
    unsigned long long wk = DC_FREE, ek = DC_FREE;
    F3 q{0.f, 0.f, 0.f};
    int s = -1;
    double cost = 0.0;
    if (a < 0 || b < 0 || a >= nv || b >= nv) {
        atomicOr(counts + 2, D3H_TOPO_ERR_RANGE);
    } else if (a != b) {
        const int ca = vclass[a], cb = vclass[b];
        int kind = 0;                                                            // 1 interior / interior, 2 interior edge with one fixed end, 3 boundary edge
        if (cnt == 2) kind = (ca == 0 && cb == 0) ? 1 : ((ca == 0) != (cb == 0) ? 2 : 0);
        else if (cnt == 1 && slide && ca == 1 && cb == 1) kind = 3;
        bool ok = kind != 0;
        if (ok) {
            Quad Qe;
            for (int k = 0; k < 10; ++k) Qe.m[k] = Q[10 * (int64_t)a + k] + Q[10 * (int64_t)b + k];
            const F3 A = dc_ld(v, a), B = dc_ld(v, b);
            const D3 Ad = dc_wide(A), Bd = dc_wide(B);
            cost = INFINITY;
            if (kind == 1) {
                const double* m = Qe.m;
                const double det = dc_det3(m[0], m[1], m[2], m[1], m[4], m[5], m[2], m[5], m[7]);
                const double t = (m[0] + m[4]) + m[7];
                const D3 mid{(Ad.x + Bd.x) * 0.5, (Ad.y + Bd.y) * 0.5, (Ad.z + Bd.z) * 0.5};
                const double r0 = -m[3], r1 = -m[6], r2 = -m[8];
                const D3 x{dc_det3(r0, m[1], m[2], r1, m[4], m[5], r2, m[5], m[7]) / det, dc_det3(m[0], r0, m[2], m[1], r1, m[5], m[2], r2, m[7]) / det,
                           dc_det3(m[0], m[1], r0, m[1], m[4], r1, m[2], m[5], r2) / det};
                const bool take = fabs(det) > DC_DET_EPS * ((t * t) * t) && __builtin_isfinite(x.x) && __builtin_isfinite(x.y) && __builtin_isfinite(x.z) &&
                                  dc_len2(x, mid) <= DC_REACH * dc_len2(Ad, Bd);
                if (take) dc_try(Qe, F3{(float)x.x, (float)x.y, (float)x.z}, cost, q);
                dc_try(Qe, F3{(float)mid.x, (float)mid.y, (float)mid.z}, cost, q);
                dc_try(Qe, A, cost, q);
                dc_try(Qe, B, cost, q);
                s = a;
            } else if (kind == 2) {
                s = ca != 0 ? a : b;
                q = ca != 0 ? A : B;
                cost = dc_error(Qe, dc_wide(q));
            } else {
                const double ea = dc_error(Qe, Ad), eb = dc_error(Qe, Bd);
                s = eb < ea ? b : a;
                q = eb < ea ? B : A;
                cost = eb < ea ? eb : ea;
            }
            ok = __builtin_isfinite(cost) && cost <= max_cost;
        }
        if (ok) {                                                                // link: interior edge two common neighbours of valence > 3, boundary edge one of valence > 2
            const int want = kind == 3 ? 1 : 2;
            int ia, ia1, ib, ib1, common = 0;
            dc_row(noffs, a, nnbr, ia, ia1);
            dc_row(noffs, b, nnbr, ib, ib1);
            while (ia < ia1 && ib < ib1) {
                const int x = nbr[ia], y = nbr[ib];
                if (x == y) {
                    ++common;
                    if (x < 0 || x >= nv || noffs[x + 1] - noffs[x] <= want + 1) ok = false;
                    ++ia, ++ib;
                } else if (x < y) {
                    ++ia;
                } else {
                    ++ib;
                }
            }
            ok = ok && common == want;
        }
        ok = ok && dc_faces_keep_normal(v, faces, idx64, nf, nv, foffs, vf, nvf, a, b, q) && dc_faces_keep_normal(v, faces, idx64, nf, nv, foffs, vf, nvf, b, a, q);
        if (ok) {
            const unsigned bits = __float_as_uint((float)cost);
            wk = ((unsigned long long)bits << 32) | (unsigned long long)(unsigned)r;
            ek = ((unsigned long long)(bits >> 20) << 32) | (unsigned long long)dc_mix((unsigned)r, round);
        }
    }
    wkey[r] = wk, ekey[r] = ek;
    eq[3 * (int64_t)r] = q.x, eq[3 * (int64_t)r + 1] = q.y, eq[3 * (int64_t)r + 2] = q.z;
    esurv[r] = s;
    ecost[r] = cost;
}

// one thread per edge: a candidate inside the window claims {a, b} + N(a) + N(b); one outside it gives its key up
__global__ __launch_bounds__(DC_T) void decim_claim_kernel(const int* __restrict__ elo, const int* __restrict__ ehi, int ne, int nv, const int* __restrict__ noffs,
                                                           const int* __restrict__ nbr, int nnbr, const unsigned long long* __restrict__ wkey,
                                                           const unsigned long long* __restrict__ wthr, unsigned long long* __restrict__ ekey,
                                                           unsigned long long* claim) {
    const int r = blockIdx.x * DC_T + threadIdx.x;
    if (r >= ne) return;
    const unsigned long long key = ekey[r];
    if (key == DC_FREE) return;
    const int a = elo[r], b = ehi[r];
    if (wkey[r] > wthr[0] || a < 0 || b < 0 || a >= nv || b >= nv) {
        ekey[r] = DC_FREE;
        return;
    }
    atomicMin(claim + a, key);
    atomicMin(claim + b, key);
    int k0, k1;
    dc_row(noffs, a, nnbr, k0, k1);
    for (int k = k0; k < k1; ++k) {
        const int j = nbr[k];
        if (j >= 0 && j < nv) atomicMin(claim + j, key);
    }
    dc_row(noffs, b, nnbr, k0, k1);
    for (int k = k0; k < k1; ++k) {
        const int j = nbr[k];
        if (j >= 0 && j < nv) atomicMin(claim + j, key);
    }
}

__device__ __forceinline__ bool dc_holds_row(const unsigned long long* __restrict__ claim, const int* __restrict__ offs, const int* __restrict__ nbr, int i,
                                             int nnbr, int nv, unsigned long long key) {
    int k0, k1;
    dc_row(offs, i, nnbr, k0, k1);
    for (int k = k0; k < k1; ++k) {
        const int j = nbr[k];
        if (j < 0 || j >= nv || claim[j] != key) return false;
    }
    return true;
}

// one thread per edge: skey = the key of a candidate that holds every claim word of its closed neighbourhood, else none
__global__ __launch_bounds__(DC_T) void decim_select_kernel(const int* __restrict__ elo, const int* __restrict__ ehi, int ne, int nv, const int* __restrict__ noffs,
                                                            const int* __restrict__ nbr, int nnbr, const unsigned long long* __restrict__ ekey,
                                                            const unsigned long long* __restrict__ claim, unsigned long long* __restrict__ skey) {
    const int r = blockIdx.x * DC_T + threadIdx.x;
    if (r >= ne) return;
    const unsigned long long key = ekey[r];
    unsigned long long out = DC_FREE;
    const int a = elo[r], b = ehi[r];
    if (key != DC_FREE && a >= 0 && b >= 0 && a < nv && b < nv && claim[a] == key && claim[b] == key && dc_holds_row(claim, noffs, nbr, a, nnbr, nv, key) &&
        dc_holds_row(claim, noffs, nbr, b, nnbr, nv, key))
        out = key;
    skey[r] = out;
}

// one thread per edge: a selected edge whose key is below the trim's cut collapses.  Reads v, Q and faces, writes vout / Qout (the caller's copies),
// remap, fdrop: selected edges have disjoint closed neighbourhoods, so no thread reads what another writes.
__global__ __launch_bounds__(DC_T) void decim_apply_kernel(const void* __restrict__ faces, int idx64, int64_t nf, int nv, const int* __restrict__ elo,
                                                           const int* __restrict__ ehi, int ne, const int* __restrict__ foffs, const int* __restrict__ vf, int nvf,
                                                           const double* __restrict__ Q, const unsigned long long* __restrict__ skey,
                                                           const unsigned long long* __restrict__ cut, const float* __restrict__ eq, const int* __restrict__ esurv,
                                                           const double* __restrict__ ecost, float* __restrict__ vout, double* __restrict__ Qout,
                                                           int* __restrict__ remap, unsigned char* __restrict__ fdrop, int* counts,
                                                           unsigned long long* maxcost) {
#pragma clang fp contract(off)
    const int r = blockIdx.x * DC_T + threadIdx.x;
    if (r >= ne) return;
    const unsigned long long key = skey[r];
    if (key == DC_FREE || !(key < cut[0])) return;
    const int a = elo[r], b = ehi[r], s = esurv[r];
    if (a < 0 || b < 0 || a >= nv || b >= nv || (s != a && s != b)) return;
    const int o = s == a ? b : a;
    vout[3 * (int64_t)s] = eq[3 * (int64_t)r], vout[3 * (int64_t)s + 1] = eq[3 * (int64_t)r + 1], vout[3 * (int64_t)s + 2] = eq[3 * (int64_t)r + 2];
    for (int k = 0; k < 10; ++k) Qout[10 * (int64_t)s + k] = Q[10 * (int64_t)a + k] + Q[10 * (int64_t)b + k];
    remap[o] = s;
    int k0, k1, dropped = 0;
    dc_row(foffs, a, nvf, k0, k1);
    for (int k = k0; k < k1; ++k) {
        const int f = vf[k];
        if (f < 0 || f >= nf) continue;
        const int64_t i0 = dc_index(faces, idx64, 3 * (int64_t)f), i1 = dc_index(faces, idx64, 3 * (int64_t)f + 1), i2 = dc_index(faces, idx64, 3 * (int64_t)f + 2);
        if (i0 == b || i1 == b || i2 == b) fdrop[f] = 1, ++dropped;
    }
    const double c = ecost[r];                                                   // finite and >= 0: its bits order as the value does
    unsigned long long bits;
    __builtin_memcpy(&bits, &c, 8);
    atomicAdd(counts, 1);
    atomicAdd(counts + 1, dropped);
    atomicMax(maxcost, bits);
}

inline bool dc_misaligned(const void* p, size_t a) { return ((uintptr_t)p & (a - 1)) != 0; }
inline unsigned dc_blocks(int64_t n) { return (unsigned)((n + DC_T - 1) / DC_T); }
inline bool dc_bad_sizes(int64_t nf, int nv, int ne, int nnbr, int nvf) {
    return nf < 0 || nf > 0x7fffffff / 3 || nv < 0 || ne < 0 || nnbr < 0 || nvf < 0;
}

}  // namespace

// Quadrics of the input mesh, one thread per vertex, no atomics.  v [nv,3] float32; faces [nf,3] int32 (idx64 = 0) or int64 (1); noffs [nv+1] / nbr
// [nnbr] int32: vertex -> neighbours CSR, ascending per vertex, ncnt [nnbr] int32 the face count of the edge to each; foffs [nv+1] / vf [nvf] int32:
// vertex -> faces CSR, ascending per vertex.  Q [nv,10] float64 overwritten: (a00, a01, a02, b0, a11, a12, b1, a22, b2, c), the sum from 0 over the
// vertex's faces in ascending index of w (u u^T, d u, d d) with n = cross(p1 - p0, p2 - p0) of the face's rows, l = sqrt(dot(n, n)) (l == 0: nothing),
// u = n / l, d = -dot(u, p0), w = l * 0.5; then, with slide != 0, over its edges of face count 1 in ascending rank the plane through the edge
// (a, b) = (min, max) perpendicular to its face: e = p[b] - p[a], m = cross(e, u), normalised (length 0: nothing), d = -dot(m, p[a]), w = 4 dot(e, e).
// counts [4] int32, accumulated: word 2 is the error word (bit 1 = an index out of range).
extern "C" int d3h_decim_quadrics(const float* v, const void* faces, int idx64, int64_t nf, int nv, const int* noffs, const int* nbr, const int* ncnt, int nnbr,
                                  const int* foffs, const int* vf, int nvf, int slide, double* Q, int* counts, void* stream) {
    if (dc_bad_sizes(nf, nv, 0, nnbr, nvf)) return D3H_ERR_ARG;
    if (nv == 0) return D3H_OK;
    if (!v || (nf > 0 && !faces) || !noffs || (nnbr > 0 && (!nbr || !ncnt)) || !foffs || (nvf > 0 && !vf) || !Q || !counts || dc_misaligned(faces, idx64 ? 8 : 4) ||
        dc_misaligned(Q, 8))
        return D3H_ERR_ARG;
    hipLaunchKernelGGL(decim_quadrics_kernel, dim3(dc_blocks(nv)), dim3(DC_T), 0, (hipStream_t)stream, v, faces, idx64, nf, nv, noffs, nbr, ncnt, nnbr, foffs, vf, nvf,
                       slide, Q, counts);
    D3H_LAUNCH_CHECK();
    return D3H_OK;
}

// Decimation round, first launch: one thread per edge.  elo / ehi / ecnt [ne] int32: the unique (min, max) edges, ascending in (min << 32 | max), and the
// face sides on each; vclass [nv] uint8: 0 interior, 1 boundary, 2 pinned; Q [nv,10] float64; max_cost: no candidate costs more; slide: boundary edges
// may collapse; round: the salt of the tie-break.  Overwritten, [ne] each: wkey uint64 = bits(float32 cost) << 32 | rank of a candidate (class,
// finite cost <= max_cost, link and normal checks passed), 0x7fff...f otherwise; ekey uint64 = (bits(float32 cost) >> 20) << 32 | mix(rank, round)
// of a candidate, 0x7fff...f otherwise; eq [ne,3] float32 the new position; esurv int32 the surviving end (-1: no class); ecost float64 the cost.
// counts [4] int32, accumulated: word 2 the error word.
extern "C" int d3h_decim_cost(const float* v, const void* faces, int idx64, int64_t nf, int nv, const int* elo, const int* ehi, const int* ecnt, int ne,
                              const int* noffs, const int* nbr, int nnbr, const int* foffs, const int* vf, int nvf, const unsigned char* vclass, const double* Q,
                              double max_cost, int slide, int round, unsigned long long* wkey, unsigned long long* ekey, float* eq, int* esurv, double* ecost,
                              int* counts, void* stream) {
    if (dc_bad_sizes(nf, nv, ne, nnbr, nvf) || round < 0 || max_cost != max_cost) return D3H_ERR_ARG;
    if (nv == 0 || ne == 0 || nf == 0) return D3H_OK;
    if (!v || !faces || !elo || !ehi || !ecnt || !noffs || (nnbr > 0 && !nbr) || !foffs || (nvf > 0 && !vf) || !vclass || !Q || !wkey || !ekey || !eq || !esurv ||
        !ecost || !counts || dc_misaligned(faces, idx64 ? 8 : 4) || dc_misaligned(Q, 8) || dc_misaligned(wkey, 8) || dc_misaligned(ekey, 8) || dc_misaligned(ecost, 8))
        return D3H_ERR_ARG;
    hipLaunchKernelGGL(decim_cost_kernel, dim3(dc_blocks(ne)), dim3(DC_T), 0, (hipStream_t)stream, v, faces, idx64, nf, nv, elo, ehi, ecnt, ne, noffs, nbr, nnbr, foffs,
                       vf, nvf, vclass, Q, max_cost, slide, (unsigned)round, wkey, ekey, eq, esurv, ecost, counts);
    D3H_LAUNCH_CHECK();
    return D3H_OK;
}

// Decimation round, second launch.  wthr [1] uint64, a DEVICE value: the window's threshold.  A candidate with wkey <= wthr puts ekey, by a 64-bit
// atomic minimum, on the claim word of every vertex of {a, b} + N(a) + N(b); one with wkey > wthr gets ekey = 0x7fff...f.  claim [nv] uint64
// overwritten (all ones where nothing claims).
extern "C" int d3h_decim_claim(const int* elo, const int* ehi, int ne, int nv, const int* noffs, const int* nbr, int nnbr, const unsigned long long* wkey,
                               const unsigned long long* wthr, unsigned long long* ekey, unsigned long long* claim, void* stream) {
    if (dc_bad_sizes(0, nv, ne, nnbr, 0)) return D3H_ERR_ARG;
    if (nv == 0 || ne == 0) return D3H_OK;
    if (!elo || !ehi || !noffs || (nnbr > 0 && !nbr) || !wkey || !wthr || !ekey || !claim || dc_misaligned(wkey, 8) || dc_misaligned(wthr, 8) ||
        dc_misaligned(ekey, 8) || dc_misaligned(claim, 8))
        return D3H_ERR_ARG;
    const hipError_t e = hipMemsetAsync(claim, 0xff, sizeof(unsigned long long) * (size_t)nv, (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(decim_claim_kernel, dim3(dc_blocks(ne)), dim3(DC_T), 0, (hipStream_t)stream, elo, ehi, ne, nv, noffs, nbr, nnbr, wkey, wthr, ekey, claim);
    D3H_LAUNCH_CHECK();
    return D3H_OK;
}

// Decimation round, third launch.  skey [ne] uint64 overwritten: ekey of a candidate that holds the claim word of its whole closed neighbourhood,
// 0x7fff...f otherwise.  Selected edges have disjoint closed neighbourhoods.
extern "C" int d3h_decim_select(const int* elo, const int* ehi, int ne, int nv, const int* noffs, const int* nbr, int nnbr, const unsigned long long* ekey,
                                const unsigned long long* claim, unsigned long long* skey, void* stream) {
    if (dc_bad_sizes(0, nv, ne, nnbr, 0)) return D3H_ERR_ARG;
    if (nv == 0 || ne == 0) return D3H_OK;
    if (!elo || !ehi || !noffs || (nnbr > 0 && !nbr) || !ekey || !claim || !skey || dc_misaligned(ekey, 8) || dc_misaligned(claim, 8) || dc_misaligned(skey, 8))
        return D3H_ERR_ARG;
    hipLaunchKernelGGL(decim_select_kernel, dim3(dc_blocks(ne)), dim3(DC_T), 0, (hipStream_t)stream, elo, ehi, ne, nv, noffs, nbr, nnbr, ekey, claim, skey);
    D3H_LAUNCH_CHECK();
    return D3H_OK;
}

// Decimation round, fourth launch.  cut [1] uint64, a DEVICE value: a selected edge with skey < cut collapses.  vout [nv,3] float32 (the caller's copy
// of v) gets eq in the survivor's row, Qout [nv,10] float64 (the caller's copy of Q) gets Q[min] + Q[max] there, remap [nv] int32 (the caller's
// identity) gets the survivor in the removed vertex's row, fdrop [nf] uint8 (the caller's zeros) gets 1 for the faces that held both ends; counts [4]
// int32, accumulated: collapses, dropped faces; maxcost [1] uint64, raised to the bits of the largest float64 cost taken (the caller's zero).
extern "C" int d3h_decim_apply(const void* faces, int idx64, int64_t nf, int nv, const int* elo, const int* ehi, int ne, const int* foffs, const int* vf, int nvf,
                               const double* Q, const unsigned long long* skey, const unsigned long long* cut, const float* eq, const int* esurv, const double* ecost,
                               float* vout, double* Qout, int* remap, unsigned char* fdrop, int* counts, unsigned long long* maxcost, void* stream) {
    if (dc_bad_sizes(nf, nv, ne, 0, nvf)) return D3H_ERR_ARG;
    if (nv == 0 || ne == 0 || nf == 0) return D3H_OK;
    if (!faces || !elo || !ehi || !foffs || (nvf > 0 && !vf) || !Q || !skey || !cut || !eq || !esurv || !ecost || !vout || !Qout || Q == Qout || !remap || !fdrop ||
        !counts || !maxcost || dc_misaligned(faces, idx64 ? 8 : 4) || dc_misaligned(Q, 8) || dc_misaligned(Qout, 8) || dc_misaligned(skey, 8) ||
        dc_misaligned(cut, 8) || dc_misaligned(ecost, 8) || dc_misaligned(maxcost, 8))
        return D3H_ERR_ARG;
    hipLaunchKernelGGL(decim_apply_kernel, dim3(dc_blocks(ne)), dim3(DC_T), 0, (hipStream_t)stream, faces, idx64, nf, nv, elo, ehi, ne, foffs, vf, nvf, Q, skey, cut, eq,
                       esurv, ecost, vout, Qout, remap, fdrop, counts, maxcost);
    D3H_LAUNCH_CHECK();
    return D3H_OK;
}
