"""Host side of csrc/meshrefine.hip: threshold edge-split refinement and Dirichlet relaxation of a triangle mesh, for the hand-off between the
split and the seq stage (the meshlabserver calls of the reference's script/process_body_cloth_head_msdfcut.py with remesh.mlx and
midpoint_head.mlx).  Tensors live on the device the kernels run on.

    refine_long_edges(v, faces, threshold, iterations=1, face_mask=None) -> (v', faces', parent)
        v [n,3] float32, faces [F,3] int32 or int64 (the result keeps the type), face_mask [F] bool / uint8 or None, parent int64 [F'].
        The refine step of isotropic remeshing and MeshLab's "Midpoint" subdivision with a threshold: conforming (no T-junction: an unmasked
        neighbour of a split edge is split too), the surface and every face's orientation are kept.  There is no collapse, flip or smoothing
        step, so short edges stay short.  One round:
          marking       an edge (min, max) is marked when min != max, (dx dx + dy dy) + dz dz > threshold * threshold with d = v[max] - v[min],
                        all in float32 without contraction, and -- with a face_mask -- at least one masked face uses it
          new vertices  the marked edges in ascending order of (min << 32 | max): edge number r gives vertex n + r at (v[min] + v[max]) * 0.5f
          child faces   face (i0, i1, i2) with edges e0 = (i0, i1), e1 = (i1, i2), e2 = (i2, i0), m_j the new vertex of e_j, k marked edges,
                        becomes k + 1 faces, the children of a parent consecutive and in parent order:
                          k = 0   (i0, i1, i2)
                          k = 1   e_j marked; a = i_j, b = i_j+1, c = i_j+2, m = m_j:     (a, m, c), (m, b, c)
                          k = 2   e_j not marked; a = i_j, b = i_j+1, c = i_j+2, p = m_j+1 on (b, c), q = m_j+2 on (c, a):
                                  the corner (p, c, q), then the quad a b p q along its shorter diagonal (squared lengths as above, of the float32
                                  positions):  |a - p|^2 < |b - q|^2: (a, b, p), (a, p, q);   |b - q|^2 < |a - p|^2: (a, b, q), (b, p, q);
                                  a tie takes the diagonal that holds the smaller original vertex: a < b the first pair, else the second
                          k = 3   (i0, m0, m2), (m0, i1, m1), (m2, m1, i2), (m0, m1, m2)
                        (j+1, j+2 modulo 3)
        Rounds repeat `iterations` times and stop once nothing is marked; a child inherits its parent's mask.  parent[i] is the INPUT face child i
        came from (through all rounds), non-decreasing: labels are carried as labels[parent].  One read-back per round (the number of marked edges,
        the number of children and the error word, together) is the only synchronisation.  A face index outside [0, n) raises.
    relax(v, faces, free_mask, iterations) -> v'
        Jacobi rounds of the uniform Laplacian: a vertex with free_mask set and at least one edge neighbour moves to the mean of its neighbours
        (the unique edges of `faces`), every other vertex is returned bit-unchanged."""
import torch

from . import _lib as L
from . import meshops as _mo
from . import meshtopo as _mt

_MAXKEY = 0x7fffffffffffffff


def _round(v, f, thr, mask):
    dev = v.device
    n, nf = int(v.shape[0]), int(f.shape[0])
    idx64 = f.dtype == torch.int64
    lg = _mt._table_log2(3 * nf, 0, 'refine_mark')
    keys = torch.empty(1 << lg, dtype=torch.int64, device=dev)
    counts = torch.empty(1 << lg, dtype=torch.int32, device=dev)
    mark = torch.empty(1 << lg, dtype=torch.int32, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    L.call('refine_mark', v, f, idx64, nf, n, mask, thr, keys, counts, mark, err)
    marked = mark > 0
    skeys = torch.sort(torch.where(marked, keys, torch.full_like(keys, _MAXKEY))).values          # the marked keys first, ascending
    nm, extra, word = torch.stack([marked.sum(), (counts.long() * marked).sum(), err[0].long()]).tolist()      # the round's one read-back
    _mt._raise(word, 'refine_long_edges')
    if nm == 0:
        return None
    skeys = skeys[:nm].contiguous()
    rank = torch.empty(nf, 3, dtype=torch.int32, device=dev)
    count = torch.empty(nf, dtype=torch.int32, device=dev)
    L.call('refine_count', f, idx64, nf, n, skeys, nm, rank, count)
    incl = torch.cumsum(count, 0, dtype=torch.int64)
    offs = (incl - count).contiguous()
    nout = nf + extra
    vout = torch.empty(n + nm, 3, dtype=torch.float32, device=dev)
    vout[:n] = v
    fout = torch.empty(nout, 3, dtype=f.dtype, device=dev)
    parent = torch.empty(nout, dtype=torch.int32, device=dev)
    L.call('refine_split', v, f, idx64, nf, n, skeys, nm, rank, offs, nout, vout, fout, parent)
    return vout, fout, parent.long()


def refine_long_edges(v, faces, threshold, iterations=1, face_mask=None):
    f = _mt._faces(faces, 'refine_long_edges')
    if v.dim() != 2 or v.shape[1] != 3 or v.dtype != torch.float32:
        raise RuntimeError(f'refine_long_edges: expected positions [n,3] float32, got {tuple(v.shape)} {v.dtype}')
    thr = float(threshold)
    if not thr >= 0.0:
        raise RuntimeError(f'refine_long_edges: the threshold must be >= 0, got {threshold}')
    v = v.detach().contiguous()
    mask = None
    if face_mask is not None:
        if face_mask.shape != (f.shape[0],) or face_mask.dtype not in (torch.bool, torch.uint8):
            raise RuntimeError(f'refine_long_edges: expected face_mask [{f.shape[0]}] bool or uint8, got {tuple(face_mask.shape)} {face_mask.dtype}')
        mask = face_mask.to(torch.uint8).contiguous()
    parent = torch.arange(f.shape[0], dtype=torch.int64, device=f.device)
    for _ in range(int(iterations)):
        if f.shape[0] == 0:
            break
        r = _round(v, f, thr, mask)
        if r is None:
            break
        v, f, p = r
        parent = parent[p]
        if mask is not None:
            mask = mask[p].contiguous()
    return v, f, parent


def relax(v, faces, free_mask, iterations):
    f = _mt._faces(faces, 'relax')
    if v.dim() != 2 or v.shape[1] != 3 or v.dtype != torch.float32:
        raise RuntimeError(f'relax: expected positions [n,3] float32, got {tuple(v.shape)} {v.dtype}')
    n, it = int(v.shape[0]), int(iterations)
    if free_mask.shape != (n,) or free_mask.dtype not in (torch.bool, torch.uint8):
        raise RuntimeError(f'relax: expected free_mask [{n}] bool or uint8, got {tuple(free_mask.shape)} {free_mask.dtype}')
    if it < 0:
        raise RuntimeError(f'relax: iterations must be >= 0, got {iterations}')
    a = v.detach().clone().contiguous()
    if n == 0 or it == 0 or f.shape[0] == 0:
        return a
    if int(f.min()) < 0 or int(f.max()) >= n:
        raise RuntimeError('relax: a face index outside [0, nv)')
    topo = _mo.EdgeTopology(_mo.find_edges(f.long()), n)
    b = torch.empty_like(a)
    L.call('relax', a, b, n, topo.offs, topo.nbr, free_mask.to(torch.uint8).contiguous(), it)
    return b if it & 1 else a
