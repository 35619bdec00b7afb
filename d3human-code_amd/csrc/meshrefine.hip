// meshrefine.hip -- threshold edge-split refinement and Dirichlet relaxation of a triangle mesh for the stage hand-off, gfx950.
//
// Replaces (reference file:line):
//   script/process_body_cloth_head_msdfcut.py:621,625,661,715  meshlabserver with checkpoints/script/remesh.mlx (the refine step of isotropic remeshing)
//   script/process_body_cloth_head_msdfcut.py:404-431          process_subdivide: meshlabserver with midpoint_head.mlx ("Midpoint" with a threshold)
//   the smoothing that screened Poisson gives the caps of a watertight mesh (wt.mlx), for d3h/watertight.py
//
// One refinement round is four launches; the host orders the marked keys between the first and the second (d3h/meshrefine.py):
//   refine_mark     one thread per (face, edge): the edge goes into an open-addressed table keyed (min << 32 | max), the table of
//                   d3h_edge_count, with the number of face sides that use it and a mark: squared length > threshold^2, the two ends differ,
//                   and -- with a face mask -- the face of this thread is masked.  Bounded probes, error word as in meshtopo.hip.
//   refine_vertices one thread per marked edge, in ascending key order: new vertex n + rank = (v[min] + v[max]) * 0.5f
//   refine_count    one thread per face: the rank of each of its edges among the sorted marked keys (binary search, -1 = not marked) and 1 + k
//   refine_split    one thread per face: its k + 1 children at the exclusive scan of the counts, and their parent
// The length test and the diagonal test are float32 with contraction off in this operation order: d = hi - lo per component, (dx dx + dy dy) + dz dz.
//
// Child table.  Face (i0, i1, i2), edges e0 = (i0, i1), e1 = (i1, i2), e2 = (i2, i0), m_j the new vertex of e_j.
//   k = 0   (i0, i1, i2)
//   k = 1   e_j marked; a = i_j, b = i_j+1, c = i_j+2, m = m_j:                    (a, m, c), (m, b, c)
//   k = 2   e_j NOT marked; a = i_j, b = i_j+1, c = i_j+2, p = m_j+1 on (b, c), q = m_j+2 on (c, a): the corner (p, c, q), then the quad
//           a b p q along its shorter diagonal -- |a - p|^2 < |b - q|^2:           (a, b, p), (a, p, q)
//           |b - q|^2 < |a - p|^2:                                                 (a, b, q), (b, p, q)
//           on a tie the diagonal with the smaller original vertex: a < b the first pair, else the second
//   k = 3   (i0, m0, m2), (m0, i1, m1), (m2, m1, i2), (m0, m1, m2)
// (indices j+1, j+2 modulo 3).  Every child keeps the parent's orientation and the children tile the parent exactly.
//
// Relaxation: Jacobi rounds of the uniform Laplacian over the CSR of unique edges (d3h/meshops.py EdgeTopology); a free vertex with neighbours
// moves to their mean, every other vertex is copied bit for bit.
#include "d3h_common.h"

#define D3H_TOPO_ERR_RANGE 1
#define D3H_TOPO_ERR_CAP 2
#define D3H_TOPO_ERR_TABLE 4

namespace {

constexpr int MR_T = 256;
constexpr unsigned long long MR_FREE = ~0ull;

__device__ __forceinline__ int64_t mr_index(const void* __restrict__ faces, int idx64, int64_t i) {
    return idx64 ? ((const int64_t*)faces)[i] : (int64_t)((const int*)faces)[i];
}

__device__ __forceinline__ unsigned long long mr_mix(unsigned long long k) {
    k ^= k >> 33; k *= 0xff51afd7ed558ccdull; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull; k ^= k >> 33;
    return k;
}

__device__ __forceinline__ unsigned long long mr_key(int64_t a, int64_t b) {
    return ((unsigned long long)(a < b ? a : b) << 32) | (unsigned long long)(a < b ? b : a);
}

// squared distance of two points, float32, no contraction: the operation order the tests restate
__device__ __forceinline__ float mr_dist2(float ax, float ay, float az, float bx, float by, float bz) {
#pragma clang fp contract(off)
    const float dx = bx - ax, dy = by - ay, dz = bz - az;
    return (dx * dx + dy * dy) + dz * dz;
}

__device__ __forceinline__ float mr_mid(float a, float b) {
#pragma clang fp contract(off)
    return (a + b) * 0.5f;
}

// one thread per (face, edge).  Ends after at most 2^log2 probes: more slots than edges, a key never leaves its slot.
__global__ __launch_bounds__(MR_T) void refine_mark_kernel(const float* __restrict__ v, const void* __restrict__ faces, int idx64, int64_t nf, int64_t nv,
                                                           const unsigned char* __restrict__ face_mask, float thr, unsigned long long* keys,
                                                           int* counts, int* mark, int log2, int* err) {
    const int64_t i = (int64_t)blockIdx.x * MR_T + threadIdx.x;
    if (i >= 3 * nf) return;
    const int64_t f = i / 3;
    const int e = (int)(i - 3 * f);
    const int64_t a = mr_index(faces, idx64, 3 * f + e), b = mr_index(faces, idx64, 3 * f + (e + 1) % 3);
    const int64_t c = mr_index(faces, idx64, 3 * f + (e + 2) % 3);
    if (a < 0 || a >= nv || b < 0 || b >= nv || c < 0 || c >= nv) {             // a face with any index out of range takes no part at all
        atomicOr(err, D3H_TOPO_ERR_RANGE);
        return;
    }
    const int64_t lo = a < b ? a : b, hi = a < b ? b : a;
    bool marked = false;
    if (lo != hi && (!face_mask || face_mask[f])) {
#pragma clang fp contract(off)
        const float thr2 = thr * thr;
        marked = mr_dist2(v[3 * lo], v[3 * lo + 1], v[3 * lo + 2], v[3 * hi], v[3 * hi + 1], v[3 * hi + 2]) > thr2;
    }
    const unsigned long long key = mr_key(a, b);
    const unsigned mask = (1u << log2) - 1u;
    unsigned slot = (unsigned)mr_mix(key) & mask;
    for (unsigned probe = 0; probe <= mask; ++probe) {
        const unsigned long long prev = atomicCAS(keys + slot, MR_FREE, key);
        if (prev == MR_FREE || prev == key) {
            atomicAdd(counts + slot, 1);
            if (marked) atomicOr(mark + slot, 1);
            return;
        }
        slot = (slot + 1) & mask;
    }
    atomicOr(err, D3H_TOPO_ERR_TABLE);
}

// one thread per marked edge, sorted[r] its key: vout row n + r
__global__ __launch_bounds__(MR_T) void refine_vertices_kernel(const float* __restrict__ v, int64_t nv, const unsigned long long* __restrict__ sorted, int64_t nm,
                                                               float* __restrict__ vout) {
    const int64_t r = (int64_t)blockIdx.x * MR_T + threadIdx.x;
    if (r >= nm) return;
    const int64_t lo = (int64_t)(sorted[r] >> 32), hi = (int64_t)(sorted[r] & 0xffffffffull);
    if (lo >= nv || hi >= nv) return;                                             // not keys of this mesh: write nothing
    for (int k = 0; k < 3; ++k) vout[3 * (nv + r) + k] = mr_mid(v[3 * lo + k], v[3 * hi + k]);
}

// rank of `key` in the ascending array sorted[nm], -1 when absent.  At most 32 halvings (nm < 2^31).
__device__ __forceinline__ int mr_rank(const unsigned long long* __restrict__ sorted, int64_t nm, unsigned long long key) {
    int64_t lo = 0, hi = nm;
    for (int step = 0; step < 32 && lo < hi; ++step) {
        const int64_t mid = (lo + hi) >> 1;
        if (sorted[mid] < key) lo = mid + 1; else hi = mid;
    }
    return (lo < nm && sorted[lo] == key) ? (int)lo : -1;
}

// one thread per face: rank[f][3] of its edges e0, e1, e2 among the marked ones (-1 = stays) and count[f] = 1 + the number marked.  A face
// with an index out of range keeps itself (count 1); the mark launch has reported it.
__global__ __launch_bounds__(MR_T) void refine_count_kernel(const void* __restrict__ faces, int idx64, int64_t nf, int64_t nv,
                                                            const unsigned long long* __restrict__ sorted, int64_t nm, int* __restrict__ rank,
                                                            int* __restrict__ count) {
    const int64_t f = (int64_t)blockIdx.x * MR_T + threadIdx.x;
    if (f >= nf) return;
    int64_t i[3];
    bool ok = true;
    for (int k = 0; k < 3; ++k) {
        i[k] = mr_index(faces, idx64, 3 * f + k);
        ok = ok && i[k] >= 0 && i[k] < nv;
    }
    int n = 1;
    for (int k = 0; k < 3; ++k) {
        const int r = (ok && i[k] != i[(k + 1) % 3]) ? mr_rank(sorted, nm, mr_key(i[k], i[(k + 1) % 3])) : -1;
        rank[3 * f + k] = r;
        n += r >= 0;
    }
    count[f] = n;
}

template <class I> __device__ __forceinline__ void mr_put(I* __restrict__ out, int* __restrict__ parent, int64_t at, int64_t a, int64_t b, int64_t c, int64_t f) {
    out[3 * at] = (I)a, out[3 * at + 1] = (I)b, out[3 * at + 2] = (I)c;
    parent[at] = (int)f;
}

// one thread per face: children at offs[f] (the exclusive scan of count), see the child table at the top of the file.  vout holds the old
// vertices and the new ones (rows nv + rank).
template <class I> __global__ __launch_bounds__(MR_T) void refine_split_kernel(const I* __restrict__ faces, int64_t nf, int64_t nv, const float* __restrict__ vout,
                                                                               const int* __restrict__ rank, const int64_t* __restrict__ offs, int64_t nout,
                                                                               I* __restrict__ out, int* __restrict__ parent) {
    const int64_t f = (int64_t)blockIdx.x * MR_T + threadIdx.x;
    if (f >= nf) return;
    const int64_t i[3] = {(int64_t)faces[3 * f], (int64_t)faces[3 * f + 1], (int64_t)faces[3 * f + 2]};
    const int r[3] = {rank[3 * f], rank[3 * f + 1], rank[3 * f + 2]};
    const int k = (r[0] >= 0) + (r[1] >= 0) + (r[2] >= 0);
    const int64_t at = offs[f];
    if (at < 0 || at + k + 1 > nout) return;                                      // not a scan of these counts: write nothing
    const int64_t m[3] = {nv + r[0], nv + r[1], nv + r[2]};
    if (k == 0) {
        mr_put(out, parent, at, i[0], i[1], i[2], f);
    } else if (k == 3) {
        mr_put(out, parent, at, i[0], m[0], m[2], f);
        mr_put(out, parent, at + 1, m[0], i[1], m[1], f);
        mr_put(out, parent, at + 2, m[2], m[1], i[2], f);
        mr_put(out, parent, at + 3, m[0], m[1], m[2], f);
    } else if (k == 1) {
        const int j = r[0] >= 0 ? 0 : (r[1] >= 0 ? 1 : 2);
        const int64_t a = i[j], b = i[(j + 1) % 3], c = i[(j + 2) % 3];
        mr_put(out, parent, at, a, m[j], c, f);
        mr_put(out, parent, at + 1, m[j], b, c, f);
    } else {
        const int j = r[0] < 0 ? 0 : (r[1] < 0 ? 1 : 2);
        const int64_t a = i[j], b = i[(j + 1) % 3], c = i[(j + 2) % 3], p = m[(j + 1) % 3], q = m[(j + 2) % 3];
        const float dap = mr_dist2(vout[3 * a], vout[3 * a + 1], vout[3 * a + 2], vout[3 * p], vout[3 * p + 1], vout[3 * p + 2]);
        const float dbq = mr_dist2(vout[3 * b], vout[3 * b + 1], vout[3 * b + 2], vout[3 * q], vout[3 * q + 1], vout[3 * q + 2]);
        const bool first = dap < dbq || (!(dbq < dap) && a < b);
        mr_put(out, parent, at, p, c, q, f);
        if (first) {
            mr_put(out, parent, at + 1, a, b, p, f);
            mr_put(out, parent, at + 2, a, p, q, f);
        } else {
            mr_put(out, parent, at + 1, a, b, q, f);
            mr_put(out, parent, at + 2, b, p, q, f);
        }
    }
}

// one Jacobi round, one thread per vertex
__global__ __launch_bounds__(MR_T) void relax_kernel(const float* __restrict__ x, float* __restrict__ y, int nv, const int* __restrict__ offs,
                                                     const int* __restrict__ nbr, const unsigned char* __restrict__ free_mask) {
    const int i = blockIdx.x * MR_T + threadIdx.x;
    if (i >= nv) return;
    const int k0 = offs[i], k1 = offs[i + 1];
    float ox = x[3 * (size_t)i], oy = x[3 * (size_t)i + 1], oz = x[3 * (size_t)i + 2];
    if (free_mask[i] && k1 > k0) {
        float sx = 0.f, sy = 0.f, sz = 0.f;
        for (int k = k0; k < k1; ++k) {
            const int j = nbr[k];
            if (j < 0 || j >= nv) continue;                                     // not an adjacency of this mesh
            sx += x[3 * (size_t)j], sy += x[3 * (size_t)j + 1], sz += x[3 * (size_t)j + 2];
        }
        const float inv = 1.0f / (float)(k1 - k0);
        ox = sx * inv, oy = sy * inv, oz = sz * inv;
    }
    y[3 * (size_t)i] = ox, y[3 * (size_t)i + 1] = oy, y[3 * (size_t)i + 2] = oz;
}

inline bool mr_misaligned(const void* p, size_t a) { return ((uintptr_t)p & (a - 1)) != 0; }
inline unsigned mr_blocks(int64_t n) { return (unsigned)((n + MR_T - 1) / MR_T); }

}  // namespace

extern "C" int d3h_topo_table_log2(int64_t items, int table_log2);              // meshtopo.hip: the table size the edge tables share

// v [nv,3] float32; faces [nf,3] int32 (idx64 = 0) or int64 (1); face_mask [nf] uint8 or NULL (every face masked); keys [2^L] uint64, counts [2^L]
// int32 and mark [2^L] int32 with L = d3h_topo_table_log2(3 nf, 0), all three overwritten: every distinct (min, max) edge in one slot with the
// number of face sides that use it and mark = 1 when it is to be split (squared length > threshold^2 in float32, ends differ, a masked face uses
// it); err [1] int32, accumulated (bits as in meshtopo.hip).
extern "C" int d3h_refine_mark(const float* v, const void* faces, int idx64, int64_t nf, int64_t nv, const unsigned char* face_mask, float threshold,
                               unsigned long long* keys, int* counts, int* mark, int* err, void* stream) {
    if (nf < 0 || nf > 0x7fffffff / 3 || nv < 0 || nv > 0x7fffffff || !(threshold >= 0.f)) return D3H_ERR_ARG;
    const int L = d3h_topo_table_log2(3 * nf, 0);
    if (L < 0 || !keys || !counts || !mark || !err || mr_misaligned(keys, 8) || mr_misaligned(counts, 4) || mr_misaligned(mark, 4) || mr_misaligned(err, 4))
        return D3H_ERR_ARG;
    if (nf > 0 && (!faces || !v || mr_misaligned(faces, idx64 ? 8 : 4) || mr_misaligned(v, 4))) return D3H_ERR_ARG;
    hipError_t e = hipMemsetAsync(keys, 0xff, sizeof(unsigned long long) << L, (hipStream_t)stream);
    if (e == hipSuccess) e = hipMemsetAsync(counts, 0, sizeof(int) << L, (hipStream_t)stream);
    if (e == hipSuccess) e = hipMemsetAsync(mark, 0, sizeof(int) << L, (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    if (nf == 0) return D3H_OK;
    hipLaunchKernelGGL(refine_mark_kernel, dim3(mr_blocks(3 * nf)), dim3(MR_T), 0, (hipStream_t)stream, v, faces, idx64, nf, nv, face_mask, threshold, keys, counts,
                       mark, L, err);
    D3H_LAUNCH_CHECK();
    return D3H_OK;
}

// sorted [nm] uint64: the marked keys of d3h_refine_mark's table, ascending (the host compacts and sorts them); rank [nf,3] int32 overwritten: the
// position of each face edge in `sorted`, -1 = not marked; count [nf] int32 overwritten: 1 + the number of marked edges = the number of children
extern "C" int d3h_refine_count(const void* faces, int idx64, int64_t nf, int64_t nv, const unsigned long long* sorted, int64_t nm, int* rank, int* count,
                                void* stream) {
    if (nf < 0 || nf > 0x7fffffff / 3 || nv < 0 || nv > 0x7fffffff || nm < 0 || nm > 0x7fffffff - nv) return D3H_ERR_ARG;
    if (nf == 0) return D3H_OK;
    if (!faces || !rank || !count || (nm > 0 && !sorted) || mr_misaligned(faces, idx64 ? 8 : 4) || mr_misaligned(sorted, 8) || mr_misaligned(rank, 4) ||
        mr_misaligned(count, 4))
        return D3H_ERR_ARG;
    hipLaunchKernelGGL(refine_count_kernel, dim3(mr_blocks(nf)), dim3(MR_T), 0, (hipStream_t)stream, faces, idx64, nf, nv, sorted, nm, rank, count);
    D3H_LAUNCH_CHECK();
    return D3H_OK;
}

// vout [nv + nm, 3] float32: rows nv.. overwritten with the midpoints (v[min] + v[max]) * 0.5f of the sorted keys (rows 0..nv-1 are the caller's copy
// of v); offs [nf] int64: the exclusive scan of d3h_refine_count's count; out [nout,3] of the faces' type and parent [nout] int32 overwritten,
// nout = the sum of count: the children of face f at offs[f].., in the order of the child table at the top of meshrefine.hip, parent = f
extern "C" int d3h_refine_split(const float* v, const void* faces, int idx64, int64_t nf, int64_t nv, const unsigned long long* sorted, int64_t nm,
                                const int* rank, const int64_t* offs, int64_t nout, float* vout, void* out, int* parent, void* stream) {
    if (nf < 0 || nf > 0x7fffffff / 3 || nv < 0 || nv > 0x7fffffff || nm < 0 || nm > 0x7fffffff - nv || nout < nf || nout > 4 * nf) return D3H_ERR_ARG;
    if (nm > 0 && (!v || !sorted || !vout || mr_misaligned(v, 4) || mr_misaligned(sorted, 8) || mr_misaligned(vout, 4))) return D3H_ERR_ARG;
    if (nf > 0 && (!faces || !rank || !offs || !out || !parent || !vout || mr_misaligned(faces, idx64 ? 8 : 4) || mr_misaligned(out, idx64 ? 8 : 4) ||
                   mr_misaligned(rank, 4) || mr_misaligned(offs, 8) || mr_misaligned(parent, 4)))
        return D3H_ERR_ARG;
    if (nm > 0) hipLaunchKernelGGL(refine_vertices_kernel, dim3(mr_blocks(nm)), dim3(MR_T), 0, (hipStream_t)stream, v, nv, sorted, nm, vout);
    if (nf > 0) {
        if (idx64)
            hipLaunchKernelGGL(refine_split_kernel<int64_t>, dim3(mr_blocks(nf)), dim3(MR_T), 0, (hipStream_t)stream, (const int64_t*)faces, nf, nv, (const float*)vout,
                               rank, offs, nout, (int64_t*)out, parent);
        else
            hipLaunchKernelGGL(refine_split_kernel<int>, dim3(mr_blocks(nf)), dim3(MR_T), 0, (hipStream_t)stream, (const int*)faces, nf, nv, (const float*)vout, rank,
                               offs, nout, (int*)out, parent);
    }
    D3H_LAUNCH_CHECK();
    return D3H_OK;
}

// `iterations` Jacobi rounds of the uniform Laplacian: a [nv,3] float32 holds the input, b [nv,3] is the second buffer; offs [nv+1] / nbr: CSR of the
// unique edges; free_mask [nv] uint8: 1 = the vertex moves to the mean of its neighbours, 0 = it is copied.  The result is in a after an even
// number of rounds and in b after an odd one.
extern "C" int d3h_relax(float* a, float* b, int nv, const int* offs, const int* nbr, const unsigned char* free_mask, int iterations, void* stream) {
    if (nv < 0 || iterations < 0 || (nv > 0 && iterations > 0 && (!a || !b || a == b || !offs || !nbr || !free_mask))) return D3H_ERR_ARG;
    if (nv == 0) return D3H_OK;
    for (int it = 0; it < iterations; ++it) {
        hipLaunchKernelGGL(relax_kernel, dim3(mr_blocks(nv)), dim3(MR_T), 0, (hipStream_t)stream, (const float*)((it & 1) ? b : a), (it & 1) ? a : b, nv, offs, nbr,
                           free_mask);
        D3H_LAUNCH_CHECK();
    }
    return D3H_OK;
}
