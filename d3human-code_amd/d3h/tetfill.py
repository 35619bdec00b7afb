"""Host side of csrc/tetfill.hip: the tetrahedra of a lattice that lie inside a surface -- what the reference gets at start-up from
script/get_tet_smpl.py (tetgen behind pyvista, geometry/hmsdf.py:239-249).  Tetgen is not rebuilt.  The substitute is a lattice clipped by the
linear interpolant of a signed distance at its vertices: its boundary is the marching-tets surface of that field, its cut vertices are marching
tets' watertight vertices bit for bit, and no vertex of the input surface is a vertex of the result.  Tensors live on the device the kernels run on.

    clip(pos, sdf, tets) -> (v [n,3] float32, t [m,4] int64, n_inside)
        pos [N,3] float32 (any strides), sdf [N] or [N,1] float32, tets [T,4] int32 or int64 indexing pos: any tet grid, any T, also 0
        side test    marching tets' own: a vertex is INSIDE when !(sdf > 0), so sdf == 0 is inside; a NaN in sdf raises ValueError
        v            the inside lattice vertices in lattice order (v[:n_inside] == pos[inside], bit for bit), then one cut vertex per
                     sign-changing edge in the order of the sorted-unique edge list of the grid (d3h.mtets.TetGrid):
                     v[n_inside:] == marching_tets(pos, sdf, ones, tets)['verts_wt'], bit for bit, same order
        t            parents in tet order, children in the order listed, 0 / 1 / 3 / 3 / 1 of them for 0 / 1 / 2 / 3 / 4 inside corners.
                     I / O = the inside / outside corners in the parent's corner order, c(i,o) = the cut vertex on edge (i,o):
                       4 inside   the parent
                       1 inside   (i, c(i,o0), c(i,o1), c(i,o2))
                       2 inside   prism [i0, c(i0,o0), c(i0,o1) | i1, c(i1,o0), c(i1,o1)]
                       3 inside   prism [i0, i1, i2 | c(i0,o), c(i1,o), c(i2,o)]
                     a prism [P0 P1 P2 | P3 P4 P5] is split smallest id first (Dompierre et al. 1999): if the smallest of the six ids is in
                     the second triangle the triangles are exchanged; both are rotated together until it is V0 (Vk pairs with Vk+3); then
                       min(V1,V5) < min(V2,V4):  (V0,V1,V2,V5) (V0,V1,V5,V4) (V0,V4,V5,V3)
                       otherwise:                (V0,V1,V2,V4) (V0,V4,V2,V5) (V0,V4,V5,V3)
                     two parents on a cut quad see the same four ids, so they cut it along the same diagonal: the result is conforming
        orientation  combinatorial, no sign test on a sliver.  PARITY by inside mask (bit k = corner k inside) is the sign of the
                     permutation (I ascending, O ascending) of the corners, 1 = odd:
                       mask    0 1 2 3 4 5 6 7 8 9 10 11 12 13 14 15
                       parity  - 0 1 0 0 1 0 0 1 0  1  1  0  0  1  0
                     a child is written with its entries 1 and 2 exchanged iff  PARITY[mask] XOR (the prism's triangles were exchanged) XOR
                     (the parent is negatively oriented: ((b-a) x (c-a)) . (d-a) < 0 in float32 -- a lattice tet is never a sliver).  Every
                     child is then positively oriented up to the rounding of its cut vertices
        all outside  empty tensors; all inside: t == tets, v == pos
        slivers      a cut arbitrarily close to a lattice vertex gives an arbitrarily thin child, and sdf == 0 at a vertex gives children of
                     zero volume.  Nothing is snapped.
    fill_mesh(verts, faces, res=64, scale=1.1, accel='brute') -> (v, t, h)
        the lattice is the cube of d3h.watertight.extract -- centred on the bounding box, side = scale x the longest extent,
        synth.kuhn_grid(res, raw=True), pitch h = side / res -- and the field is meshops.mesh_wsdf: on a closed mesh mesh_sdf's bits; an open,
        consistently wound garment gets its holes closed at |w| = 0.5.  accel='bvh': the field by meshops.mesh_wsdf(accel='bvh'), from a tree

One call of clip launches up to three kernels (an emit without output is skipped) and reads the three sizes and the error word back once,
between the first and the second.  A bad shape or dtype and a tet index outside [0, N) raise RuntimeError before any launch."""
import torch

from . import _lib as L
from . import meshops as _mo
from . import mtets as _mtets

ERR_NAN = 1


def clip(pos, sdf, tets):
    if pos.dim() != 2 or pos.shape[1] != 3 or pos.dtype != torch.float32:
        raise RuntimeError(f'clip: expected positions [N,3] float32, got {tuple(pos.shape)} {pos.dtype}')
    n = int(pos.shape[0])
    if sdf.dtype != torch.float32 or sdf.numel() != n or sdf.dim() not in (1, 2):
        raise RuntimeError(f'clip: expected sdf [{n}] float32, got {tuple(sdf.shape)} {sdf.dtype}')
    if tets.dim() != 2 or tets.shape[1] != 4 or tets.dtype not in (torch.int32, torch.int64):
        raise RuntimeError(f'clip: expected tets [T,4] int32 or int64, got {tuple(tets.shape)} {tets.dtype}')
    nt = int(tets.shape[0])
    if nt >= 1 << 29 or n >= 1 << 31:
        raise RuntimeError(f'clip: {nt} tets / {n} vertices: more than int32 indices hold')
    if nt > 0 and (int(tets.min()) < 0 or int(tets.max()) >= n):
        raise RuntimeError('clip: a tet index outside [0, N)')
    pos = pos.detach().contiguous()
    sdf = sdf.detach().reshape(-1).contiguous()
    dev = pos.device
    g = _mtets.TetGrid.get(tets)
    ne = g.ne
    nb = lambda k: max(1, (k + 255) // 256)
    nbv, nbe, nbt = nb(n), nb(ne), nb(nt)
    blk = torch.empty(nbv + nbe + nbt, dtype=torch.int32, device=dev)
    blk_v, blk_e, blk_t = blk[:nbv], blk[nbv:nbv + nbe], blk[nbv + nbe:]
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    L.call('tetfill_count', sdf, n, g.tets32, nt, g.edges32, ne, blk_v, blk_e, blk_t, err)
    incl = [torch.cumsum(b, 0) for b in (blk_v, blk_e, blk_t)]
    off_v, off_e, off_t = [(c - b).int() for c, b in zip(incl, (blk_v, blk_e, blk_t))]
    n_in, n_cut, m, word = torch.stack([incl[0][-1], incl[1][-1], incl[2][-1], err[0].long()]).tolist()          # the one read-back
    if word & ERR_NAN:
        raise ValueError('clip: a NaN in sdf')
    v = torch.empty(n_in + n_cut, 3, dtype=torch.float32, device=dev)
    t = torch.empty(m, 4, dtype=torch.int64, device=dev)
    vert_id = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    edge_vid = torch.empty(max(ne, 1), dtype=torch.int32, device=dev)
    if n_in + n_cut > 0:
        L.call('tetfill_emit_verts', pos, sdf, n, g.edges32, ne, off_v, off_e, n_in, vert_id, edge_vid, v)
    if m > 0:
        L.call('tetfill_emit_tets', pos, sdf, g.tets32, g.tet_edge32, nt, off_t, vert_id, edge_vid, t)
    return v, t, n_in


def fill_mesh(verts, faces, res=64, scale=1.1, accel='brute'):
    from . import watertight as _wt
    v = verts.detach().contiguous().float()
    if v.dim() != 2 or v.shape[1] != 3 or v.shape[0] == 0 or faces.dim() != 2 or faces.shape[1] != 3 or faces.shape[0] == 0:
        raise RuntimeError(f'fill_mesh: expected a mesh v [n,3], f [F,3] with n, F > 0, got {tuple(v.shape)} {tuple(faces.shape)}')
    lo, hi = v.min(0).values, v.max(0).values
    side = float((hi - lo).max()) * float(scale)
    if not side > 0.0:
        raise RuntimeError('fill_mesh: the mesh has no extent')
    unit, tets = _wt._lattice(res, v.device)                              # [-1, 1]^3
    pos = ((lo + hi) * 0.5 + unit * (side * 0.5)).contiguous()
    sdf, _ = _mo.mesh_wsdf(pos, v, faces, want_w=False, accel=accel)
    out_v, out_t, _ = clip(pos, sdf, tets)
    return out_v, out_t, side / int(res)
