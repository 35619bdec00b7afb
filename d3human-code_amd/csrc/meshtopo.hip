// meshtopo.hip -- mesh topology between the training stages: connected components, exact vertex weld, open-edge detection, gfx950.
//
// Replaces (reference file:line):
//   script/connet_face_head.py:19-74,83-86   UnionFind + find_connected_components (Python lists, one interpreter step per face)
//   script/connet_face_head.py:97-112        merge_and_repair_meshes -> open3d remove_duplicated_vertices (exact coordinates, first
//                                            occurrence kept, order kept) + remove_degenerate_triangles (the latter is host-side torch)
//   script/process_body_cloth_head_msdfcut.py:92-102  find_open_edges (torch.unique over the 3F sorted edges, counts == 1)
//
// All three groups are lock-free: no thread ever waits for another thread to act.  Every loop ends by an invariant that is stated at the
// loop, and carries an iteration cap derived from that invariant; a thread that reaches the cap sets a bit of the caller's error word
// and leaves (a wrong kernel must end, not spin).  The error word is an int32 in device memory:
//   D3H_TOPO_ERR_RANGE (1)  a face index outside [0, nv): that face / edge was skipped
//   D3H_TOPO_ERR_CAP   (2)  an iteration cap was reached (never, if the invariants hold)
//   D3H_TOPO_ERR_TABLE (4)  a probe sequence went once round the hash table without finding its key or a free slot
// Nothing here synchronises; the caller reads the error word back when it needs the result.  Scalars are written with ordinary stores.
//
// Connected components.  parent[nv] is a union-find forest with ONE invariant: parent[x] <= x at all times, and a value only ever goes
// down (every write is an atomicMin or a compare-and-swap from x to something smaller).  So a chain x, parent[x], parent[parent[x]], ...
// strictly descends until it meets a root (parent[r] == r): no cycles, at most nv steps.  A root is hooked under a SMALLER root only,
// by compare-and-swap on its own cell; when the swap fails some other thread has hooked that root in the meantime (the forest lost a
// root: at most nv - 1 such events in the whole launch), and the thread finds the two roots again.  When the launch is over, the root of
// a tree is the smallest vertex index of its component whatever the schedule was, so the labels are deterministic.
//
// Weld.  An open-addressed table of 2^table_log2 > n int32 slots, -1 = free.  A slot holds a vertex index and that vertex's coordinates
// are the slot's key; atomicMin between indices of equal coordinates never changes the key, so probe sequences stay valid while the
// table fills.  A slot never becomes free again.  More slots than rows: a probe meets its key or a free slot within one revolution.
//
// Open edges.  The same table over 64-bit keys (min << 32 | max) with an int counter per slot.
#include "d3h_common.h"

#define D3H_TOPO_ERR_RANGE 1
#define D3H_TOPO_ERR_CAP 2
#define D3H_TOPO_ERR_TABLE 4

namespace {

constexpr int MT_T = 256;
constexpr int MT_MAX_LOG2 = 30;                 // 2^30 int32 slots = 4 GiB; indices and slot numbers stay inside int32
constexpr unsigned long long MT_FREE = ~0ull;

__device__ __forceinline__ int64_t mt_index(const void* __restrict__ faces, int idx64, int64_t i) {
    return idx64 ? ((const int64_t*)faces)[i] : (int64_t)((const int*)faces)[i];
}

// a load that is not kept in a register or a stale line of the compute unit's own cache while other threads update the cell
__device__ __forceinline__ int mt_load(const int* p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }

__device__ __forceinline__ unsigned long long mt_mix(unsigned long long k) {
    k ^= k >> 33; k *= 0xff51afd7ed558ccdull; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull; k ^= k >> 33;
    return k;
}

// ---- connected components --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MT_T) void cc_init_kernel(int* __restrict__ parent, int64_t nv, int* __restrict__ err) {
    const int64_t i = (int64_t)blockIdx.x * MT_T + threadIdx.x;
    if (i == 0) err[0] = 0;
    if (i < nv) parent[i] = (int)i;
}

// root of x, halving the path on the way.  Ends because the chain strictly descends (parent[y] < y for every y that is not a root);
// `cap` = nv + 1 steps cannot be reached.  -1 when it is.
__device__ __forceinline__ int cc_find(int* parent, int x, int64_t cap, int* err) {
    for (int64_t step = 0; step < cap; ++step) {
        const int p = mt_load(parent + x);
        if (p == x) return x;
        if (p < 0 || p > x) break;                     // not a forest this file built: do not follow it
        const int g = mt_load(parent + p);
        if (g != p) atomicMin(parent + x, g);          // g <= p < x: the cell only goes down, and g is an ancestor of x
        x = p;
    }
    atomicOr(err, D3H_TOPO_ERR_CAP);
    return -1;
}

// Ends because every failed compare-and-swap means that another thread hooked a root since this thread's find: the forest loses a root each
// time, nv - 1 times at the most in the whole launch, so `cap` = nv + 1 rounds cannot be reached.
__device__ __forceinline__ void cc_unite(int* parent, int a, int b, int64_t cap, int* err) {
    for (int64_t round = 0; round < cap; ++round) {
        a = cc_find(parent, a, cap, err);
        b = cc_find(parent, b, cap, err);
        if (a < 0 || b < 0 || a == b) return;
        const int hi = a > b ? a : b, lo = a > b ? b : a;
        if (atomicCAS(parent + hi, hi, lo) == hi) return;          // the larger root goes under the smaller one
    }
    atomicOr(err, D3H_TOPO_ERR_CAP);
}

// one thread per face: edges (0,1) and (1,2), as the reference's loop
__global__ __launch_bounds__(MT_T) void cc_hook_kernel(const void* __restrict__ faces, int idx64, int64_t nf, int* parent, int64_t nv, int* err) {
    const int64_t f = (int64_t)blockIdx.x * MT_T + threadIdx.x;
    if (f >= nf) return;
    const int64_t i0 = mt_index(faces, idx64, 3 * f), i1 = mt_index(faces, idx64, 3 * f + 1), i2 = mt_index(faces, idx64, 3 * f + 2);
    if (i0 < 0 || i0 >= nv || i1 < 0 || i1 >= nv || i2 < 0 || i2 >= nv) {
        atomicOr(err, D3H_TOPO_ERR_RANGE);
        return;
    }
    cc_unite(parent, (int)i0, (int)i1, nv + 1, err);
    cc_unite(parent, (int)i1, (int)i2, nv + 1, err);
}

// one thread per vertex, after the hook launch: the forest no longer changes.  Ends because the chain strictly descends (cap nv + 1).
__global__ __launch_bounds__(MT_T) void cc_flatten_kernel(const int* __restrict__ parent, int64_t nv, int* __restrict__ label, int* err) {
    const int64_t v = (int64_t)blockIdx.x * MT_T + threadIdx.x;
    if (v >= nv) return;
    int x = (int)v;
    for (int64_t step = 0; step <= nv; ++step) {
        const int p = parent[x];
        if (p == x) { label[v] = x; return; }
        if (p < 0 || p > x) break;                                   // not a forest this file built: do not follow it
        x = p;
    }
    label[v] = (int)v;
    atomicOr(err, D3H_TOPO_ERR_CAP);
}

// ---- weld ------------------------------------------------------------------------------------------------------------------------
template <class T> struct MtBits;
template <> struct MtBits<float> { typedef unsigned type; };
template <> struct MtBits<double> { typedef unsigned long long type; };

template <class T> struct MtRow {
    T x, y, z;
    bool nan;
    unsigned long long hash;
};

// equality is by value in T: -0 == +0, so the hash takes +0 for both; a row with a NaN equals nothing
template <class T> __device__ __forceinline__ MtRow<T> mt_row(const T* __restrict__ pos, int64_t i) {
    MtRow<T> r;
    r.x = pos[3 * i], r.y = pos[3 * i + 1], r.z = pos[3 * i + 2];
    r.nan = r.x != r.x || r.y != r.y || r.z != r.z;
    T c[3] = {r.x, r.y, r.z};
    unsigned long long h = 0x9e3779b97f4a7c15ull;
    for (int k = 0; k < 3; ++k) {
        if (c[k] == (T)0) c[k] = (T)0;
        typename MtBits<T>::type b;
        __builtin_memcpy(&b, &c[k], sizeof(T));
        h = mt_mix(h ^ (unsigned long long)b);
    }
    r.hash = h;
    return r;
}

template <class T> __device__ __forceinline__ bool mt_same(const MtRow<T>& r, const T* __restrict__ pos, int j) {
    return r.x == pos[3 * (int64_t)j] && r.y == pos[3 * (int64_t)j + 1] && r.z == pos[3 * (int64_t)j + 2];
}

// one thread per row.  Ends after at most 2^log2 probes: the table has more slots than rows and a slot never becomes free again, so one
// revolution meets the row's key or a free slot.
template <class T> __global__ __launch_bounds__(MT_T) void weld_insert_kernel(const T* __restrict__ pos, int64_t n, int* table, int log2, int* err) {
    const int64_t i = (int64_t)blockIdx.x * MT_T + threadIdx.x;
    if (i >= n) return;
    const MtRow<T> r = mt_row(pos, i);
    if (r.nan) return;                                              // equals nothing: never looked for, so it needs no slot
    const unsigned mask = (1u << log2) - 1u;
    unsigned slot = (unsigned)r.hash & mask;
    for (unsigned probe = 0; probe <= mask; ++probe) {
        int cur = mt_load(table + slot);
        if (cur == -1) {
            cur = atomicCAS(table + slot, -1, (int)i);
            if (cur == -1) return;                                  // the slot is this row's now
        }                                                           // a failed swap returned the owner: the same slot, now taken
        if (cur < 0 || cur >= n) break;                             // not a table this launch filled
        if (mt_same(r, pos, cur)) {
            atomicMin(table + slot, (int)i);                        // equal coordinates: the key stays, the lowest index wins
            return;
        }
        slot = (slot + 1) & mask;
    }
    atomicOr(err, D3H_TOPO_ERR_TABLE);
}

// rep[i] = the lowest index with row i's coordinates (i itself for a row with a NaN).  Same probe sequence, same bound.
template <class T> __global__ __launch_bounds__(MT_T) void weld_lookup_kernel(const T* __restrict__ pos, int64_t n, const int* __restrict__ table, int log2,
                                                                              int* __restrict__ rep, int* err) {
    const int64_t i = (int64_t)blockIdx.x * MT_T + threadIdx.x;
    if (i >= n) return;
    rep[i] = (int)i;
    const MtRow<T> r = mt_row(pos, i);
    if (r.nan) return;
    const unsigned mask = (1u << log2) - 1u;
    unsigned slot = (unsigned)r.hash & mask;
    for (unsigned probe = 0; probe <= mask; ++probe) {
        const int cur = table[slot];
        if (cur < 0 || cur >= n) break;                             // a free slot before the key: the row was never inserted
        if (mt_same(r, pos, cur)) { rep[i] = cur; return; }
        slot = (slot + 1) & mask;
    }
    atomicOr(err, D3H_TOPO_ERR_TABLE);
}

// ---- open edges ------------------------------------------------------------------------------------------------------------------
// one thread per (face, edge): edges (0,1), (1,2), (2,0), each as (min, max).  An edge (a,a) is counted like any other.  Ends after at most
// 2^log2 probes: more slots than edges, a key never leaves its slot.
__global__ __launch_bounds__(MT_T) void edge_count_kernel(const void* __restrict__ faces, int idx64, int64_t nf, int64_t nv, unsigned long long* keys,
                                                          int* counts, int log2, int* err) {
    const int64_t i = (int64_t)blockIdx.x * MT_T + threadIdx.x;
    if (i >= 3 * nf) return;
    const int64_t f = i / 3;
    const int e = (int)(i - 3 * f);
    const int64_t a = mt_index(faces, idx64, 3 * f + e), b = mt_index(faces, idx64, 3 * f + (e + 1) % 3);
    if (a < 0 || a >= nv || b < 0 || b >= nv) {
        atomicOr(err, D3H_TOPO_ERR_RANGE);
        return;
    }
    const unsigned long long key = ((unsigned long long)(a < b ? a : b) << 32) | (unsigned long long)(a < b ? b : a);
    const unsigned mask = (1u << log2) - 1u;
    unsigned slot = (unsigned)mt_mix(key) & mask;
    for (unsigned probe = 0; probe <= mask; ++probe) {
        const unsigned long long prev = atomicCAS(keys + slot, MT_FREE, key);
        if (prev == MT_FREE || prev == key) {
            atomicAdd(counts + slot, 1);
            return;
        }
        slot = (slot + 1) & mask;
    }
    atomicOr(err, D3H_TOPO_ERR_TABLE);
}

// one thread per slot: both ends of an edge that exactly one face side uses
__global__ __launch_bounds__(MT_T) void open_vertex_mask_kernel(const unsigned long long* __restrict__ keys, const int* __restrict__ counts, int64_t slots,
                                                                int64_t nv, unsigned char* __restrict__ mask) {
    const int64_t s = (int64_t)blockIdx.x * MT_T + threadIdx.x;
    if (s >= slots) return;
    const unsigned long long k = keys[s];
    if (k == MT_FREE || counts[s] != 1) return;
    const int64_t lo = (int64_t)(k >> 32), hi = (int64_t)(k & 0xffffffffull);
    if (lo >= nv || hi >= nv) return;
    mask[lo] = 1;
    mask[hi] = 1;
}

inline bool mt_misaligned(const void* p, size_t a) { return ((uintptr_t)p & (a - 1)) != 0; }
inline unsigned mt_blocks(int64_t n) { return (unsigned)((n + MT_T - 1) / MT_T); }

}  // namespace

// log2 of the table a call with `items` keys and this `table_log2` uses: 0 asks for the default, the smallest power of two >= 2 items;
// any other value is taken when 2^table_log2 > items (and <= 2^30).  D3H_ERR_ARG otherwise.  Host arithmetic only.
extern "C" int d3h_topo_table_log2(int64_t items, int table_log2) {
    if (items < 0 || items >= ((int64_t)1 << MT_MAX_LOG2) || table_log2 < 0 || table_log2 > MT_MAX_LOG2) return D3H_ERR_ARG;
    if (table_log2 == 0) {
        int l = 0;
        while (((int64_t)1 << l) < 2 * items) ++l;
        return l > MT_MAX_LOG2 ? D3H_ERR_ARG : l;
    }
    return ((int64_t)1 << table_log2) > items ? table_log2 : D3H_ERR_ARG;
}

// parent [nv] int32, overwritten with the identity; err [1] int32, overwritten with 0 (the error word of the three cc calls, bits above)
extern "C" int d3h_cc_init(int* parent, int64_t nv, int* err, void* stream) {
    if (nv < 0 || nv > 0x7fffffff || !err || (nv > 0 && !parent) || mt_misaligned(parent, 4) || mt_misaligned(err, 4)) return D3H_ERR_ARG;
    hipLaunchKernelGGL(cc_init_kernel, dim3(nv ? mt_blocks(nv) : 1u), dim3(MT_T), 0, (hipStream_t)stream, parent, nv, err);
    D3H_LAUNCH_CHECK();
    return D3H_OK;
}

// faces [nf,3] int32 (idx64 = 0) or int64 (idx64 = 1): unites the ends of edges (0,1) and (1,2) of every face in `parent` (as d3h_cc_init left
// it, or after earlier hook calls).  A face with repeated indices is legal; one with an index outside [0, nv) is skipped and reported in err.
extern "C" int d3h_cc_hook(const void* faces, int idx64, int64_t nf, int* parent, int64_t nv, int* err, void* stream) {
    if (nf < 0 || nf > 0x7fffffff || nv < 0 || nv > 0x7fffffff || !err || mt_misaligned(err, 4)) return D3H_ERR_ARG;
    if (nf == 0) return D3H_OK;
    if (!faces || (nv > 0 && !parent) || mt_misaligned(faces, idx64 ? 8 : 4) || mt_misaligned(parent, 4)) return D3H_ERR_ARG;
    hipLaunchKernelGGL(cc_hook_kernel, dim3(mt_blocks(nf)), dim3(MT_T), 0, (hipStream_t)stream, faces, idx64, nf, parent, nv, err);
    D3H_LAUNCH_CHECK();
    return D3H_OK;
}

// label [nv] int32, overwritten: the root of every vertex = the smallest vertex index of its component (an isolated vertex: itself)
extern "C" int d3h_cc_flatten(const int* parent, int64_t nv, int* label, int* err, void* stream) {
    if (nv < 0 || nv > 0x7fffffff || !err || mt_misaligned(err, 4)) return D3H_ERR_ARG;
    if (nv == 0) return D3H_OK;
    if (!parent || !label || mt_misaligned(parent, 4) || mt_misaligned(label, 4)) return D3H_ERR_ARG;
    hipLaunchKernelGGL(cc_flatten_kernel, dim3(mt_blocks(nv)), dim3(MT_T), 0, (hipStream_t)stream, parent, nv, label, err);
    D3H_LAUNCH_CHECK();
    return D3H_OK;
}

// pos [n,3] float32 (f64 = 0) or float64 (f64 = 1); table [2^L] int32 with L = d3h_topo_table_log2(n, table_log2), overwritten (filled with -1
// here, then with the rows); err [1] int32, accumulated (the caller zero-fills).
extern "C" int d3h_weld_insert(const void* pos, int f64, int64_t n, int* table, int table_log2, int* err, void* stream) {
    const int L = d3h_topo_table_log2(n, table_log2);
    if (L < 0 || !table || !err || mt_misaligned(table, 4) || mt_misaligned(err, 4)) return D3H_ERR_ARG;
    if (n > 0 && (!pos || mt_misaligned(pos, f64 ? 8 : 4))) return D3H_ERR_ARG;
    hipError_t e = hipMemsetAsync(table, 0xff, sizeof(int) << L, (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    if (n == 0) return D3H_OK;
    if (f64) hipLaunchKernelGGL(weld_insert_kernel<double>, dim3(mt_blocks(n)), dim3(MT_T), 0, (hipStream_t)stream, (const double*)pos, n, table, L, err);
    else hipLaunchKernelGGL(weld_insert_kernel<float>, dim3(mt_blocks(n)), dim3(MT_T), 0, (hipStream_t)stream, (const float*)pos, n, table, L, err);
    D3H_LAUNCH_CHECK();
    return D3H_OK;
}

// rep [n] int32, overwritten: the lowest index whose row equals row i, from the table d3h_weld_insert filled with the same pos / n / table_log2
extern "C" int d3h_weld_lookup(const void* pos, int f64, int64_t n, const int* table, int table_log2, int* rep, int* err, void* stream) {
    const int L = d3h_topo_table_log2(n, table_log2);
    if (L < 0 || !table || !err || mt_misaligned(table, 4) || mt_misaligned(err, 4)) return D3H_ERR_ARG;
    if (n == 0) return D3H_OK;
    if (!pos || !rep || mt_misaligned(pos, f64 ? 8 : 4) || mt_misaligned(rep, 4)) return D3H_ERR_ARG;
    if (f64) hipLaunchKernelGGL(weld_lookup_kernel<double>, dim3(mt_blocks(n)), dim3(MT_T), 0, (hipStream_t)stream, (const double*)pos, n, table, L, rep, err);
    else hipLaunchKernelGGL(weld_lookup_kernel<float>, dim3(mt_blocks(n)), dim3(MT_T), 0, (hipStream_t)stream, (const float*)pos, n, table, L, rep, err);
    D3H_LAUNCH_CHECK();
    return D3H_OK;
}

// faces [nf,3] int32 / int64; keys [2^L] uint64 and counts [2^L] int32 with L = d3h_topo_table_log2(3 nf, table_log2), both overwritten: every
// distinct (min, max) edge in one slot with the number of face sides that use it; err [1] int32, accumulated.
extern "C" int d3h_edge_count(const void* faces, int idx64, int64_t nf, int64_t nv, unsigned long long* keys, int* counts, int table_log2, int* err,
                              void* stream) {
    if (nf < 0 || nf > 0x7fffffff / 3 || nv < 0 || nv > 0x7fffffff) return D3H_ERR_ARG;
    const int L = d3h_topo_table_log2(3 * nf, table_log2);
    if (L < 0 || !keys || !counts || !err || mt_misaligned(keys, 8) || mt_misaligned(counts, 4) || mt_misaligned(err, 4)) return D3H_ERR_ARG;
    if (nf > 0 && (!faces || mt_misaligned(faces, idx64 ? 8 : 4))) return D3H_ERR_ARG;
    hipError_t e = hipMemsetAsync(keys, 0xff, sizeof(unsigned long long) << L, (hipStream_t)stream);
    if (e == hipSuccess) e = hipMemsetAsync(counts, 0, sizeof(int) << L, (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    if (nf == 0) return D3H_OK;
    hipLaunchKernelGGL(edge_count_kernel, dim3(mt_blocks(3 * nf)), dim3(MT_T), 0, (hipStream_t)stream, faces, idx64, nf, nv, keys, counts, L, err);
    D3H_LAUNCH_CHECK();
    return D3H_OK;
}

// mask [nv] uint8, overwritten: 1 for both ends of every edge of the table (L = its log2 size, as resolved by d3h_edge_count) whose count is
// exactly 1, 0 elsewhere.  An edge of three or more face sides is not open.
extern "C" int d3h_open_vertex_mask(const unsigned long long* keys, const int* counts, int table_log2, int64_t nv, unsigned char* mask, void* stream) {
    if (table_log2 < 0 || table_log2 > MT_MAX_LOG2 || nv < 0 || nv > 0x7fffffff || !keys || !counts || mt_misaligned(keys, 8) || mt_misaligned(counts, 4))
        return D3H_ERR_ARG;
    if (nv == 0) return D3H_OK;
    if (!mask) return D3H_ERR_ARG;
    hipError_t e = hipMemsetAsync(mask, 0, (size_t)nv, (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    const int64_t slots = (int64_t)1 << table_log2;
    hipLaunchKernelGGL(open_vertex_mask_kernel, dim3(mt_blocks(slots)), dim3(MT_T), 0, (hipStream_t)stream, keys, counts, slots, nv, mask);
    D3H_LAUNCH_CHECK();
    return D3H_OK;
}
