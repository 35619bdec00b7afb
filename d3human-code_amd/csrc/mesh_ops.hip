// mesh_ops.hip -- seq-stage geometry regularisers on a fixed-topology mesh, gfx950.
//
// Replaces (reference file:line):
//   render/mesh.py:30-82 compute_laplacian_uniform + lap_loss.py:40-47 body_laplacian_loss    mean_i |(L V)_i|^2, L = D^-1 A - I
//   render/mesh.py:18-28,266-279 normal_consistency_loss (lap_loss.py:50-55 body_normal_loss)  mean (1 - cos(n_a, n_b))^2
//   geometry/hmsdf.py:98-132 collision_loss                                                     mean relu(eps - (p - c_f) . n_f)^2
//   geometry/hmsdf.py:236-237 pysdf.SDF(template)(grid vertices) of the SDF pre-fit             signed distance to a closed mesh
// The reference rebuilds a sparse V x V matrix from the edge list on every call (mesh.py:259-263 recomputes the property each
// time) and runs a sparse mm; the topology is static in this stage, so the host builds a CSR adjacency once and both L V and its
// transpose are atomic-free gathers.  All three are HBM/latency-bound passes over 10^4-10^5 elements.
#include "d3h_meshdist_dev.h"

namespace {

// mode 0: out_i = inv_deg_i * sum_{j in N(i)} x_j - x_i                 (L x)
// mode 1: out_i = sum_{j in N(i)} inv_deg_j * s * x_j - s * x_i          (L^T (s x)), s = scale[0] * post
// sumsq (mode 0, optional): += sum_i |out_i|^2
__global__ __launch_bounds__(256) void uniform_laplacian_kernel(const float* __restrict__ x, int nv, const int* __restrict__ offs,
                                                                const int* __restrict__ nbr, const float* __restrict__ inv_deg, int mode,
                                                                const float* __restrict__ scale, float post, float* __restrict__ out,
                                                                float* __restrict__ sumsq) {
    __shared__ float s4[4];
    int i = blockIdx.x * 256 + threadIdx.x;
    float sq = 0.f;
    if (i < nv) {
        V3 acc = mk(0.f, 0.f, 0.f);
        for (int k = offs[i]; k < offs[i + 1]; ++k) {
            int j = nbr[k];
            V3 xj = ld3(x + 3 * (size_t)j);
            acc = acc + (mode ? xj * inv_deg[j] : xj);
        }
        V3 xi = ld3(x + 3 * (size_t)i);
        V3 o = mode ? (acc - xi) * (scale[0] * post) : acc * inv_deg[i] - xi;
        st3(out + 3 * (size_t)i, o);
        sq = dot(o, o);
    }
    if (sumsq) {
        float tot = block_sum(sq, s4);
        if (threadIdx.x == 0) atomicAdd(sumsq, tot);
    }
}

__device__ __forceinline__ V3 face_cross(const float* __restrict__ v, const int* __restrict__ f, int t, int (&id)[3], V3 (&p)[3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) { id[k] = f[3 * (size_t)t + k]; p[k] = ld3(v + 3 * (size_t)id[k]); }
    return cross(p[1] - p[0], p[2] - p[0]);
}
// d(cross(p1-p0, p2-p0)) chain: given g = dL/dn, scatter to the three vertices
__device__ __forceinline__ void face_cross_bwd(const V3 (&p)[3], const int (&id)[3], V3 g, float* __restrict__ d_v) {
    V3 e1 = p[1] - p[0], e2 = p[2] - p[0];
    V3 g1 = cross(e2, g), g2 = cross(g, e1);          // dL/de1 = e2 x g, dL/de2 = g x e1
    atomic_add3(d_v + 3 * (size_t)id[1], g1);
    atomic_add3(d_v + 3 * (size_t)id[2], g2);
    atomic_add3(d_v + 3 * (size_t)id[0], (g1 + g2) * -1.f);
}

// torch.cosine_similarity: (a / max(|a|, 1e-8)) . (b / max(|b|, 1e-8))
__global__ __launch_bounds__(256) void normal_consistency_kernel(const float* __restrict__ v, const int* __restrict__ f, const int* __restrict__ pairs,
                                                                 int np, const float* __restrict__ g_scalar, float post, float* __restrict__ sum,
                                                                 float* __restrict__ d_v) {
    __shared__ float s4[4];
    int i = blockIdx.x * 256 + threadIdx.x;
    float val = 0.f;
    if (i < np) {
        int ia[3], ib[3];
        V3 pa[3], pb[3];
        V3 na = face_cross(v, f, pairs[2 * (size_t)i], ia, pa), nb = face_cross(v, f, pairs[2 * (size_t)i + 1], ib, pb);
        float la, lb;
        V3 a = normalize_eps(na, 1e-8f, la), b = normalize_eps(nb, 1e-8f, lb);
        float c = dot(a, b);
        val = (1.0f - c) * (1.0f - c);
        if (d_v) {
            float gc = -2.0f * (1.0f - c) * g_scalar[0] * post;
            face_cross_bwd(pa, ia, normalize_eps_bwd(a, la, 1e-8f, b * gc), d_v);
            face_cross_bwd(pb, ib, normalize_eps_bwd(b, lb, 1e-8f, a * gc), d_v);
        }
    }
    if (sum) {
        float tot = block_sum(val, s4);
        if (threadIdx.x == 0) atomicAdd(sum, tot);
    }
}

// one cloth vertex per thread; nn[i] = nearest body face (by centre); F.normalize eps 1e-12 on the face normal
__global__ __launch_bounds__(256) void collision_kernel(const float* __restrict__ cloth, int nc, const float* __restrict__ body, const int* __restrict__ bf,
                                                        const int* __restrict__ nn, float push_eps, const float* __restrict__ g_scalar, float post,
                                                        float* __restrict__ sum, float* __restrict__ d_cloth, float* __restrict__ d_body) {
    __shared__ float s4[4];
    int i = blockIdx.x * 256 + threadIdx.x;
    float val = 0.f;
    if (i < nc) {
        int id[3];
        V3 p[3];
        V3 n = face_cross(body, bf, nn[i], id, p);
        float ln;
        V3 nh = normalize_eps(n, 1e-12f, ln);
        V3 c = (p[0] + p[1] + p[2]) * (1.0f / 3.0f);
        V3 x = ld3(cloth + 3 * (size_t)i);
        V3 dir = x - c;
        float pen = push_eps - dot(dir, nh);
        if (pen > 0.f) {
            val = pen * pen;
            if (d_cloth || d_body) {
                float gd = -2.0f * pen * g_scalar[0] * post;          // dL/d(distance)
                if (d_cloth) st3(d_cloth + 3 * (size_t)i, nh * gd);
                if (d_body) {
                    V3 gc = nh * (-gd * (1.0f / 3.0f));
#pragma unroll
                    for (int k = 0; k < 3; ++k) atomic_add3(d_body + 3 * (size_t)id[k], gc);
                    face_cross_bwd(p, id, normalize_eps_bwd(nh, ln, 1e-12f, dir * gd), d_body);
                }
            }
        } else if (d_cloth) {
            st3(d_cloth + 3 * (size_t)i, mk(0.f, 0.f, 0.f));
        }
    }
    if (sum) {
        float tot = block_sum(val, s4);
        if (threadIdx.x == 0) atomicAdd(sum, tot);
    }
}

__global__ void face_centers_kernel(const float* __restrict__ v, const int* __restrict__ f, int nf, float* __restrict__ c) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nf) return;
    V3 a = ld3(v + 3 * (size_t)f[3 * (size_t)i]), b = ld3(v + 3 * (size_t)f[3 * (size_t)i + 1]), d = ld3(v + 3 * (size_t)f[3 * (size_t)i + 2]);
    st3(c + 3 * (size_t)i, (a + b + d) * (1.0f / 3.0f));
}

// ---- signed distance of query points to a closed triangle mesh ---------------------------------------------------------------
// Replaces pysdf.SDF(template)(grid_vertices) of the SDF pre-fit (geometry/hmsdf.py:236-237, CPU, third party): exact unsigned
// distance (closest point on every triangle, Ericson's region test) and the sign from the generalised winding number (sum of the
// triangles' solid angles, van Oosterom-Strackee: robust for any closed, consistently wound mesh).  Brute force, one thread per query,
// triangles staged through LDS as (v0, e1, e2): 262 144 queries x 20 908 SMPL-X faces = 5.5e9 pairs, start-up only.
constexpr int MSDF_TILE = 1024;

// tri_dist2, vos_term, wsdf_angle_f64: d3h_meshdist_dev.h (shared with the BVH queries of bvhdist.hip)

__global__ __launch_bounds__(256) void mesh_sdf_kernel(const float* __restrict__ pts, int np, const float* __restrict__ v, const int* __restrict__ f,
                                                       int nf, float* __restrict__ out) {
    __shared__ float tri[MSDF_TILE * 9];
    const int i = blockIdx.x * 256 + threadIdx.x;
    V3 p = mk(0.f, 0.f, 0.f);
    if (i < np) p = ld3(pts + 3 * (size_t)i);
    float best = INFINITY, wind = 0.f;
    for (int base = 0; base < nf; base += MSDF_TILE) {
        const int cnt = min(MSDF_TILE, nf - base);
        __syncthreads();
        for (int t = threadIdx.x; t < cnt; t += 256) {
            const int* ff = f + 3 * (size_t)(base + t);
            V3 a = ld3(v + 3 * (size_t)ff[0]), b = ld3(v + 3 * (size_t)ff[1]), c = ld3(v + 3 * (size_t)ff[2]);
            st3(tri + 9 * t, a); st3(tri + 9 * t + 3, b - a); st3(tri + 9 * t + 6, c - a);
        }
        __syncthreads();
        for (int t = 0; t < cnt; ++t) {
            V3 a = ld3(tri + 9 * t), ab = ld3(tri + 9 * t + 3), ac = ld3(tri + 9 * t + 6);
            best = fminf(best, tri_dist2(p, a, ab, ac));
            const VosTerm s = vos_term(p, a, ab, ac);
            wind += 2.0f * atan2f(s.det, s.den);
        }
    }
    // winding number 1 inside an outward-wound closed mesh; positive OUTSIDE, negative inside (= -pysdf, the sign hmsdf.py:237 uses)
    if (i < np) out[i] = (fabsf(wind) > 6.2831853f ? -1.0f : 1.0f) * sqrtf(best);
}

// ---- winding-signed distance to an OPEN (or closed) triangle mesh --------------------------------------------------------------
// The stage hand-off's distance oracle (script/process_body_cloth_head_msdfcut.py:613-747 makes the garment watertight with screened
// Poisson and asks pysdf): the same loop as mesh_sdf_kernel, with the winding number itself as a second output.  w = solid-angle sum
// / 4 pi, in turns; sdf = (|w| > 0.5 ? -1 : +1) * distance to the nearest triangle, the test made on the radian sum exactly as
// mesh_sdf_kernel makes it, so that a closed mesh gives mesh_sdf's bits (a query within rounding of an edge or a vertex of the mesh excepted, where
// the triangles it lies on are evaluated in float64, see the loop, and mesh_sdf's float32 residue may put the sign of a zero distance either way).  For an open, consistently wound mesh the |w| = 0.5 surface closes the holes.
// Either output may be NULL.
__global__ __launch_bounds__(256) void mesh_wsdf_kernel(const float* __restrict__ pts, int np, const float* __restrict__ v, const int* __restrict__ f,
                                                        int nf, float* __restrict__ out_sdf, float* __restrict__ out_w) {
    __shared__ float tri[MSDF_TILE * 9];
    const int i = blockIdx.x * 256 + threadIdx.x;
    V3 p = mk(0.f, 0.f, 0.f);
    if (i < np) p = ld3(pts + 3 * (size_t)i);
    float best = INFINITY, wind = 0.f, fix = 0.f;
    for (int base = 0; base < nf; base += MSDF_TILE) {
        const int cnt = min(MSDF_TILE, nf - base);
        __syncthreads();
        for (int t = threadIdx.x; t < cnt; t += 256) {
            const int* ff = f + 3 * (size_t)(base + t);
            V3 a = ld3(v + 3 * (size_t)ff[0]), b = ld3(v + 3 * (size_t)ff[1]), c = ld3(v + 3 * (size_t)ff[2]);
            st3(tri + 9 * t, a); st3(tri + 9 * t + 3, b - a); st3(tri + 9 * t + 6, c - a);
        }
        __syncthreads();
        for (int t = 0; t < cnt; ++t) {
            V3 a = ld3(tri + 9 * t), ab = ld3(tri + 9 * t + 3), ac = ld3(tri + 9 * t + 6);
            best = fminf(best, tri_dist2(p, a, ab, ac));
            const VosTerm s = vos_term(p, a, ab, ac);
            // A query within rounding of the triangle's plane (a point ON the mesh: a vertex of it, a point of an edge): det, and on an edge den too, are
            // rounding residue in float32, and the residue would decide between 0 and +-half a turn.  That triangle alone is evaluated in float64 from
            // the vertices themselves (the staged edges are already rounded); everything else stays mesh_sdf_kernel's arithmetic.
            // `wind` itself is mesh_sdf_kernel's sum, untouched; `fix` collects what the repaired triangles change.
            const float ang = 2.0f * atan2f(s.det, s.den);
            wind += ang;
            if (fabsf(s.det) < 1e-4f * s.lll) fix += wsdf_angle_f64(p, v, f + 3 * (size_t)(base + t)) - ang;
        }
    }
    if (i >= np) return;
    // Within 1e-3 rad of the decision itself (a query ON a face of a closed mesh: half a turn exactly) either side is right: mesh_sdf_kernel's is taken.
    const float rep = wind + fix;
    const bool inside = fabsf(fabsf(rep) - 6.2831853f) < 1e-3f ? fabsf(wind) > 6.2831853f : fabsf(rep) > 6.2831853f;
    if (out_sdf) out_sdf[i] = (inside ? -1.0f : 1.0f) * sqrtf(best);
    if (out_w) out_w[i] = rep * 0.079577472f;                                           // 1 / (4 pi)
}

// ---- collision push: one Jacobi round of deform_body_collision (script/process_body_cloth_head_msdfcut.py:337-347) ---------------
// v[i] -= n[i] / (|n[i]| + 1e-7) * eps wherever sdf_in[i] < margin (sdf_in positive INSIDE, pysdf's sign, taken by the caller before the
// round).  A vertex whose normal has length 0 (one that no face uses) would be displaced by nothing: it is left alone and not counted, so that it cannot
// keep the caller's rounds going.  moved[0] += the number of vertices pushed (one atomic per wave); pushes[i] += 1 for each of them (optional).
__global__ __launch_bounds__(256) void collision_push_kernel(float* __restrict__ v, const float* __restrict__ n, const float* __restrict__ sdf_in, int nv,
                                                             float margin, float eps, int* __restrict__ moved, int* __restrict__ pushes) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    bool push = i < nv && sdf_in[i] < margin;
    V3 nn = mk(0.f, 0.f, 0.f);
    if (push) {
        nn = ld3(n + 3 * (size_t)i);
        push = dot(nn, nn) > 0.f;
    }
    if (push) {
        V3 u = nn * (1.0f / (sqrtf(dot(nn, nn)) + 1e-7f));
        st3(v + 3 * (size_t)i, ld3(v + 3 * (size_t)i) - u * eps);
        if (pushes) pushes[i] += 1;
    }
    const unsigned long long b = __ballot(push);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(moved, (int)__popcll(b));
}

inline dim3 grid256(int64_t n) { return dim3((unsigned)((n + 255) / 256)); }

}  // namespace

// ------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------
// CSR adjacency of the mesh's unique edges: offs[nv+1], nbr[2 ne]; inv_deg[nv] = 1/deg (0 for isolated vertices).
// lv[nv][3] = L v (kept for the backward); sumsq[0] (zeroed here) = sum_i |lv_i|^2
extern "C" int d3h_laplacian_loss_fwd(const float* v, int nv, const int* offs, const int* nbr, const float* inv_deg, float* lv, float* sumsq,
                                      void* stream) {
    if (nv < 0 || (nv > 0 && (!v || !offs || !nbr || !inv_deg || !lv)) || !sumsq) return D3H_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    (void)hipMemsetAsync(sumsq, 0, sizeof(float), s);
    if (nv > 0) hipLaunchKernelGGL(uniform_laplacian_kernel, grid256(nv), dim3(256), 0, s, v, nv, offs, nbr, inv_deg, 0, (const float*)nullptr, 1.0f, lv, sumsq);
    D3H_LAUNCH_CHECK();
    return D3H_OK;
}
// d_v[nv][3] = L^T (g_scalar[0] * post * lv)   (post = 2 / nv for the mean of squared norms); overwritten
extern "C" int d3h_laplacian_loss_bwd(const float* lv, int nv, const int* offs, const int* nbr, const float* inv_deg, const float* g_scalar,
                                      float post, float* d_v, void* stream) {
    if (nv < 0 || (nv > 0 && (!lv || !offs || !nbr || !inv_deg || !g_scalar || !d_v))) return D3H_ERR_ARG;
    if (nv > 0) hipLaunchKernelGGL(uniform_laplacian_kernel, grid256(nv), dim3(256), 0, (hipStream_t)stream, lv, nv, offs, nbr, inv_deg, 1, g_scalar, post, d_v,
                                   (float*)nullptr);
    D3H_LAUNCH_CHECK();
    return D3H_OK;
}

// pairs[np][2]: face ids sharing an edge (Mesh.connected_faces); sum[0] (zeroed here) = sum (1 - cos)^2
extern "C" int d3h_normal_consistency_fwd(const float* v, const int* f, const int* pairs, int np, float* sum, void* stream) {
    if (np < 0 || !sum || (np > 0 && (!v || !f || !pairs))) return D3H_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    (void)hipMemsetAsync(sum, 0, sizeof(float), s);
    if (np > 0) hipLaunchKernelGGL(normal_consistency_kernel, grid256(np), dim3(256), 0, s, v, f, pairs, np, (const float*)nullptr, 0.f, sum, (float*)nullptr);
    D3H_LAUNCH_CHECK();
    return D3H_OK;
}
// d_v is ACCUMULATED into (caller zero-fills); gradient of g_scalar[0] * post * sum
extern "C" int d3h_normal_consistency_bwd(const float* v, const int* f, const int* pairs, int np, const float* g_scalar, float post, float* d_v,
                                          void* stream) {
    if (np < 0 || (np > 0 && (!v || !f || !pairs || !g_scalar || !d_v))) return D3H_ERR_ARG;
    if (np > 0) hipLaunchKernelGGL(normal_consistency_kernel, grid256(np), dim3(256), 0, (hipStream_t)stream, v, f, pairs, np, g_scalar, post, (float*)nullptr, d_v);
    D3H_LAUNCH_CHECK();
    return D3H_OK;
}

// centres[nf][3] of the triangles f (int32) over v
extern "C" int d3h_face_centers(const float* v, const int* f, int nf, float* centers, void* stream) {
    if (nf < 0 || (nf > 0 && (!v || !f || !centers))) return D3H_ERR_ARG;
    if (nf > 0) hipLaunchKernelGGL(face_centers_kernel, grid256(nf), dim3(256), 0, (hipStream_t)stream, v, f, nf, centers);
    D3H_LAUNCH_CHECK();
    return D3H_OK;
}
// nn[nc]: nearest body face of each cloth vertex (d3h_knn1 against d3h_face_centers); sum[0] (zeroed here) = sum relu(eps - d)^2
extern "C" int d3h_collision_fwd(const float* cloth, int nc, const float* body, const int* body_faces, const int* nn, float push_eps, float* sum,
                                 void* stream) {
    if (nc < 0 || !sum || (nc > 0 && (!cloth || !body || !body_faces || !nn))) return D3H_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    (void)hipMemsetAsync(sum, 0, sizeof(float), s);
    if (nc > 0) hipLaunchKernelGGL(collision_kernel, grid256(nc), dim3(256), 0, s, cloth, nc, body, body_faces, nn, push_eps, (const float*)nullptr, 0.f, sum,
                                   (float*)nullptr, (float*)nullptr);
    D3H_LAUNCH_CHECK();
    return D3H_OK;
}
// d_cloth[nc][3] overwritten (may be NULL); d_body accumulated into (caller zero-fills; may be NULL); gradient of g_scalar[0] * post * sum
extern "C" int d3h_collision_bwd(const float* cloth, int nc, const float* body, const int* body_faces, const int* nn, float push_eps,
                                 const float* g_scalar, float post, float* d_cloth, float* d_body, void* stream) {
    if (nc < 0 || (nc > 0 && (!cloth || !body || !body_faces || !nn || !g_scalar))) return D3H_ERR_ARG;
    if (nc > 0) hipLaunchKernelGGL(collision_kernel, grid256(nc), dim3(256), 0, (hipStream_t)stream, cloth, nc, body, body_faces, nn, push_eps, g_scalar, post,
                                   (float*)nullptr, d_cloth, d_body);
    D3H_LAUNCH_CHECK();
    return D3H_OK;
}

// out[np]: signed distance (positive outside, negative inside) of pts[np][3] to the closed triangle mesh (v, f int32 [nf][3])
extern "C" int d3h_mesh_sdf(const float* pts, int np, const float* v, const int* f, int nf, float* out, void* stream) {
    if (np < 0 || nf <= 0 || (np > 0 && (!pts || !v || !f || !out))) return D3H_ERR_ARG;
    if (np > 0) hipLaunchKernelGGL(mesh_sdf_kernel, grid256(np), dim3(256), 0, (hipStream_t)stream, pts, np, v, f, nf, out);
    D3H_LAUNCH_CHECK();
    return D3H_OK;
}

// out_sdf[np] (may be NULL): (|w| > 0.5 ? -1 : +1) * distance of pts[np][3] to the nearest triangle of the mesh (v, f int32 [nf][3]), which may be
// open; out_w[np] (may be NULL): the generalised winding number in turns.  A closed mesh gives out_sdf == d3h_mesh_sdf's out, bit for bit (but for the sign
// of a zero distance at a query on the mesh's own edges: the triangles a query lies on are evaluated in float64).
extern "C" int d3h_mesh_wsdf(const float* pts, int np, const float* v, const int* f, int nf, float* out_sdf, float* out_w, void* stream) {
    if (np < 0 || nf <= 0 || (np > 0 && (!pts || !v || !f))) return D3H_ERR_ARG;
    if (np > 0 && (out_sdf || out_w)) hipLaunchKernelGGL(mesh_wsdf_kernel, grid256(np), dim3(256), 0, (hipStream_t)stream, pts, np, v, f, nf, out_sdf, out_w);
    D3H_LAUNCH_CHECK();
    return D3H_OK;
}

// one round of the hand-off's collision push: v[nv][3] updated in place, v[i] -= n[i] / (|n[i]| + 1e-7) * eps where sdf_in[i] < margin (sdf_in[nv]
// positive inside) and n[i] is not the zero vector; moved[1] int32 accumulated with the number of vertices pushed; pushes[nv] int32 (may be NULL) += 1 for
// each of them
extern "C" int d3h_collision_push(float* v, const float* n, const float* sdf_in, int nv, float margin, float eps, int* moved, int* pushes, void* stream) {
    if (nv < 0 || !moved || (nv > 0 && (!v || !n || !sdf_in))) return D3H_ERR_ARG;
    if (nv > 0) hipLaunchKernelGGL(collision_push_kernel, grid256(nv), dim3(256), 0, (hipStream_t)stream, v, n, sdf_in, nv, margin, eps, moved, pushes);
    D3H_LAUNCH_CHECK();
    return D3H_OK;
}
