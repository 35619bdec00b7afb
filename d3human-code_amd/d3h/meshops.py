"""Host side of csrc/mesh_ops.hip: the seq-stage geometry regularisers on a fixed-topology mesh.

    laplacian_loss(v, topo)                  render/mesh.py:30-82 + lap_loss.py:40-47   mean |L V|^2, uniform Laplacian
    normal_consistency(v, faces32, pairs32)  render/mesh.py:18-28,266-279               mean (1 - cos)^2 over connected faces
    collision_loss(cloth, body, faces, eps)  geometry/hmsdf.py:98-132                   mean relu(eps - (p - c_f) . n_f)^2
    find_edges / find_connected_faces        render/mesh.py:85-134                      vectorised, on the tensors' device

`EdgeTopology` holds what the reference rebuilds from the edge list on every call (degree, adjacency): built once per edge tensor."""
import torch

from . import _lib as L
from . import lbs as _lbs


def find_edges(indices, remove_duplicates=True):
    e = torch.cat([indices[:, [0, 1]], indices[:, [1, 2]], indices[:, [2, 0]]], dim=1).view(indices.shape[0] * 3, 2)
    if remove_duplicates:
        e = torch.unique(torch.sort(e, dim=1).values, dim=0)
    return e


def find_connected_faces(indices):
    """mesh.py:106-134 without the per-edge Python loop: (pairs [E,2] of faces sharing an edge, first-seen face first, rows in ascending
    edge order; all 3F sorted edges).  Raises like the reference's assert when an edge has more than two faces."""
    e = torch.sort(find_edges(indices, remove_duplicates=False), dim=1).values
    _, inv, counts = torch.unique(e, dim=0, return_inverse=True, return_counts=True)
    if int(counts.max()) != 2:
        raise AssertionError('find_connected_faces: non-manifold or open edge (mesh.py:116 asserts counts.max() == 2)')
    face_ids = torch.arange(indices.shape[0], device=indices.device).repeat_interleave(3)
    order = torch.argsort(inv, stable=True)
    starts = torch.cumsum(counts, 0) - counts
    two = counts == 2
    pairs = torch.stack([face_ids[order[starts[two]]], face_ids[order[starts[two] + 1]]], dim=1)
    return pairs, e


class EdgeTopology:
    """CSR adjacency + 1/degree of a unique undirected edge list [E,2] over nv vertices (compute_laplacian_uniform's A and deg)"""
    _cache = {}

    def __init__(self, edges, nv):
        dev = edges.device
        e = edges.long()
        src = torch.cat([e[:, 0], e[:, 1]])
        dst = torch.cat([e[:, 1], e[:, 0]])
        order = torch.argsort(src, stable=True)
        deg = torch.bincount(src, minlength=nv)
        self.nv = nv
        self.offs = torch.cat([torch.zeros(1, dtype=torch.long, device=dev), torch.cumsum(deg, 0)]).int().contiguous()
        self.nbr = dst[order].int().contiguous()
        degf = deg.float()
        self.inv_deg = torch.where(degf > 0, 1.0 / degf, degf).contiguous()

    @classmethod
    def get(cls, edges, nv):
        k = (edges.data_ptr(), tuple(edges.shape), nv, str(edges.device))
        t = cls._cache.get(k)
        if t is None or t[0] is not edges:
            if len(cls._cache) > 16:
                cls._cache.clear()
            t = (edges, cls(edges, nv))
            cls._cache[k] = t
        return t[1]


class _LaplacianLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, v, topo):
        vc = v.contiguous().float()
        nv = vc.shape[0]
        lv = torch.empty_like(vc)
        s = torch.empty(1, dtype=torch.float32, device=vc.device)
        L.call('laplacian_loss_fwd', vc, nv, topo.offs, topo.nbr, topo.inv_deg, lv, s)
        ctx.save_for_backward(lv)
        ctx.topo = topo
        return s[0] / nv

    @staticmethod
    def backward(ctx, g):
        lv, = ctx.saved_tensors
        topo = ctx.topo
        nv = lv.shape[0]
        d_v = torch.empty_like(lv)
        gs = g.reshape(1).contiguous().float()
        L.call('laplacian_loss_bwd', lv, nv, topo.offs, topo.nbr, topo.inv_deg, gs, 2.0 / nv, d_v)
        return d_v, None


def laplacian_loss(v, edges):
    """lap_loss.py:40-47 body_laplacian_loss: mean over vertices of |(L V)_i|^2 with mesh.py:30-82's uniform Laplacian"""
    return _LaplacianLossFn.apply(v, EdgeTopology.get(edges, v.shape[0]))


class _NormalConsistencyFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, v, faces32, pairs32):
        vc = v.contiguous().float()
        n = pairs32.shape[0]
        s = torch.empty(1, dtype=torch.float32, device=vc.device)
        L.call('normal_consistency_fwd', vc, faces32, pairs32, n, s)
        ctx.save_for_backward(vc, faces32, pairs32)
        return s[0] / n

    @staticmethod
    def backward(ctx, g):
        vc, faces32, pairs32 = ctx.saved_tensors
        n = pairs32.shape[0]
        d_v = L.zeros_like(vc)
        gs = g.reshape(1).contiguous().float()
        L.call('normal_consistency_bwd', vc, faces32, pairs32, n, gs, 1.0 / n, d_v)
        return d_v, None, None


def normal_consistency(v, faces32, pairs32):
    """mesh.py:18-28: mean (1 - cos(n_a, n_b))^2 over connected faces, n = cross(v1 - v0, v2 - v0) (un-normalised, mesh.py:242-254)"""
    return _NormalConsistencyFn.apply(v, faces32, pairs32)


class _CollisionFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cloth, body, faces32, push_eps):
        cc, bc = cloth.contiguous().float(), body.contiguous().float()
        nc, nf = cc.shape[0], faces32.shape[0]
        centers = torch.empty(nf, 3, dtype=torch.float32, device=cc.device)
        L.call('face_centers', bc, faces32, nf, centers)
        nn = _lbs.knn1(cc, centers)                      # knn_points(cloth, centres, K=1): squared L2, first minimum wins
        s = torch.empty(1, dtype=torch.float32, device=cc.device)
        L.call('collision_fwd', cc, nc, bc, faces32, nn, push_eps, s)
        ctx.save_for_backward(cc, bc, faces32, nn)
        ctx.eps = float(push_eps)
        return s[0] / nc

    @staticmethod
    def backward(ctx, g):
        cc, bc, faces32, nn = ctx.saved_tensors
        nc = cc.shape[0]
        d_c = torch.empty_like(cc) if ctx.needs_input_grad[0] else None
        d_b = L.zeros_like(bc) if ctx.needs_input_grad[1] else None
        gs = g.reshape(1).contiguous().float()
        L.call('collision_bwd', cc, nc, bc, faces32, nn, ctx.eps, gs, 1.0 / nc, d_c, d_b)
        return d_c, d_b, None, None


def collision_loss(cloth_pos, body_pos, body_faces, push_eps=0.005):
    """geometry/hmsdf.py:98-132"""
    if body_faces.shape[0] == 3 and body_faces.ndim == 2 and body_faces.shape[1] != 3:
        body_faces = body_faces.T                                    # hmsdf.py:104-105
    f32 = body_faces if body_faces.dtype == torch.int32 else body_faces.int()
    return _CollisionFn.apply(cloth_pos, body_pos, f32.contiguous(), push_eps)


def mesh_sdf(points, verts, faces):
    """signed distance (positive OUTSIDE, negative inside) of points [n,3] to the closed, consistently wound triangle mesh
    (verts [V,3], faces [F,3]): what the SDF pre-fit gets as `-pysdf.SDF(verts, faces)(points)` in the reference (hmsdf.py:236-237)"""
    p = points.detach().contiguous().float()
    v = verts.detach().contiguous().float()
    f = faces if faces.dtype == torch.int32 else faces.int()
    out = torch.empty(p.shape[0], dtype=torch.float32, device=p.device)
    L.call('mesh_sdf', p, p.shape[0], v, f.contiguous(), f.shape[0], out)
    return out


ACCELS = ('brute', 'bvh')


def mesh_wsdf(points, verts, faces, want_sdf=True, want_w=True, check=True, accel='brute', beta=3.0, bvh=None):
    """-> (sdf, w) of points [n,3] against the triangle mesh (verts [V,3], faces [F,3], F > 0), which may be OPEN: w is the generalised winding
    number in turns (solid-angle sum / 4 pi), sdf = (|w| > 0.5 ? -1 : +1) * distance to the nearest triangle.  A triangle whose plane the query lies in
    to within rounding (a query ON the mesh) is evaluated in float64, so that w does not hang on float32 residue there.  On a closed mesh sdf is
    mesh_sdf, bit for bit; on an open, consistently wound one the |w| = 0.5 surface closes the holes.  An output that is not wanted is None.
    check=False skips the range check of the faces (two read-backs) for a caller that has made it, such as a field queried every round.
    accel='brute' (the default) is the loop over every triangle, one thread per query.  accel='bvh' answers from a d3h.raytrace.Bvh -- `bvh` if one is
    passed (built over these verts and faces: a field queried every round builds once), a fresh one otherwise: O(log F) per query, the same
    per-triangle arithmetic, the winding number by the tree with the opening parameter `beta` (raytrace.Bvh.winding; beta=inf the exact sum in tree
    order).  The distance is the brute-force route's minimum unless the mesh has zero-area triangles, which the tree never returns; w, and with it the
    sign near |w| = 0.5, carries the approximation's error."""
    if accel not in ACCELS:
        raise RuntimeError(f'mesh_wsdf: accel must be one of {ACCELS}, got {accel!r}')
    p = points.detach().contiguous().float()
    v = verts.detach().contiguous().float()
    if p.dim() != 2 or p.shape[1] != 3 or v.dim() != 2 or v.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3:
        raise RuntimeError(f'mesh_wsdf: expected points [n,3], verts [V,3], faces [F,3], got {tuple(p.shape)} {tuple(v.shape)} {tuple(faces.shape)}')
    f = (faces if faces.dtype == torch.int32 else faces.int()).contiguous()
    if check and f.shape[0] > 0 and (int(f.min()) < 0 or int(f.max()) >= v.shape[0]):
        raise RuntimeError('mesh_wsdf: a face index outside [0, V)')
    if accel == 'bvh':
        from . import raytrace as _rt
        if bvh is None:
            bvh = _rt.Bvh(v, f)
        elif not isinstance(bvh, _rt.Bvh) or bvh.F != f.shape[0]:
            raise RuntimeError('mesh_wsdf: bvh must be a raytrace.Bvh built over these verts and faces')
        if not (want_sdf or want_w):
            return None, None
        return bvh._wsdf('mesh_wsdf', p, beta, want_sdf, want_w)
    sdf = torch.empty(p.shape[0], dtype=torch.float32, device=p.device) if want_sdf else None
    w = torch.empty(p.shape[0], dtype=torch.float32, device=p.device) if want_w else None
    L.call('mesh_wsdf', p, p.shape[0], v, f, f.shape[0], sdf, w)
    return sdf, w


def collision_push(v, normals, field, eps=0.005, margin=0.002, rounds=100, stop_when_still=True):
    """the reference's deform_body_collision (script/process_body_cloth_head_msdfcut.py:331-349) as Jacobi rounds on the device: each round takes
    sdf_in = field(v) once (positive INSIDE, pysdf's sign; `field` maps a float32 [n,3] device tensor to [n]), then v[i] -= n[i] / (|n[i]| + 1e-7) * eps
    wherever sdf_in[i] < margin and n[i] is not zero (a zero normal would move the vertex by nothing).  Stops when a round moves nothing (one count read-back per round) or after `rounds`.
    -> (v', pushes int32 [n]: how often each vertex moved)"""
    x = v.detach().clone().contiguous().float()
    nrm = normals.detach().contiguous().float()
    n = x.shape[0]
    pushes = torch.zeros(n, dtype=torch.int32, device=x.device)
    moved = torch.zeros(1, dtype=torch.int32, device=x.device)
    for _ in range(int(rounds)):
        s = field(x).contiguous().float()
        moved.zero_()
        L.call('collision_push', x, nrm, s, n, margin, eps, moved, pushes)
        if stop_when_still and int(moved.item()) == 0:
            break
    return x, pushes
