"""Host side of csrc/meshrefine.hip: threshold edge-split refinement and Dirichlet relaxation of a triangle mesh, for the hand-off between the
split and the seq stage (the meshlabserver calls of the reference's script/process_body_cloth_head_msdfcut.py with remesh.mlx and
midpoint_head.mlx).  Tensors live on the device the kernels run on.

    refine_long_edges(v, faces, threshold, iterations=1, face_mask=None) -> (v', faces', parent)
        v [n,3] float32, faces [F,3] int32 or int64 (the result keeps the type), face_mask [F] bool / uint8 or None, parent int64 [F'].
        The refine step of isotropic remeshing and MeshLab's "Midpoint" subdivision with a threshold: conforming (no T-junction: an unmasked
        neighbour of a split edge is split too), the surface and every face's orientation are kept.  There is no collapse, flip or smoothing
        step here, so short edges stay short (isotropic_remesh below adds them).  One round:
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
        (the unique edges of `faces`), every other vertex is returned bit-unchanged.

The other steps of isotropic remeshing (csrc/meshremesh.hip), all opt-in.  Shared conventions:
    arithmetic    float32, every operation rounded once in the order written, no contraction:  len2(a, b) = (dx dx + dy dy) + dz dz with d = b - a;
                  dot(u, w) = (ux wx + uy wy) + uz wz;  cross(u, w) = (uy wz - uz wy, uz wx - ux wz, ux wy - uy wx);  nrm(p0, p1, p2) =
                  cross(p1 - p0, p2 - p0), for a face its stored rows in order;  the cosine test  cos(n, m) >= c  is  d = dot(n, m); d > 0 and
                  d d >= c2 (dot(n, n) dot(m, m)),  c2 = c^2 a float32 constant (0.25 or 0.75)
    adjacency     rebuilt with torch sorts at the start of every round from the faces as they stand: the unique (min, max) edges in ascending
                  (min << 32 | max) order with the face sides on each -- an edge's RANK is its position --, the neighbours of each vertex (the other
                  ends of its edges with min != max) ascending, the faces of each vertex ascending; the valence is the number of neighbours
    pinned        a vertex on an edge that is not used by exactly two face sides (boundary, non-manifold), or one pin_mask [n] (bool / uint8) sets.
                  Pinned vertices never move and never disappear: open boundaries and non-manifold spots come back bit-unchanged
    selection     every candidate puts its key, by a 64-bit atomic minimum, on one claim word per vertex of its claim set and is SELECTED when it
                  holds all of them: the smallest key wins, which does not depend on the order of arrival, and selected operations touch disjoint
                  data, so every output is bit-reproducible.  The kernels' counters and the error word come back in one read-back per round.
    validation    as refine_long_edges: shapes and dtypes, a face index outside [0, n) raises, F = 0 returns the input

    collapse_short_edges(v, faces, lo, hi, rounds=8, pin_mask=None) -> (v', f', parent, vmap)
        One round.  Edge (a, b) = (min, max) is a candidate when its face count is 2, a != b, a and b are not both pinned, len2(v[a], v[b]) < lo lo
        and all of these hold on the round's input (they are tested BEFORE the claims: a short edge that fails them would otherwise win its
        neighbourhood in every round and keep every collapsible edge near it waiting for ever):
          link      N(a) and N(b) share exactly two vertices and both have valence > 3 (else a tetrahedron would collapse to a two-faced fin)
          position  q = the pinned end's position if one is pinned, else (v[a] + v[b]) * 0.5f
          length    len2(q, v[x]) <= hi hi for every x of N(a) + N(b) other than a, b (a following split must not undo the collapse)
          normal    every face that holds a or b but not both passes the cosine test at c2 = 0.25 (60 degrees) between nrm of its rows and nrm of
                    its rows with the end replaced by q
        key = bits(len2) << 32 | rank (the shortest wins, ties to the smaller rank); claim set {a, b} + N(a) + N(b), so selected edges have disjoint
        closed neighbourhoods and every selected edge collapses.  The survivor s is the pinned end, else a: v[s] = q, the other end is renumbered s, the two faces that held both are dropped.
        v' = v without the removed vertices (order kept; unreferenced vertices stay), f' = the kept faces in order, renumbered, in the input's type,
        parent int64 [F'] = the input face of each, vmap int64 [n] = old index -> new index (a removed vertex -> its survivor).  Up to `rounds`
        rounds; a round that collapses nothing ends the loop.
    flip_edges(v, faces, rounds=8, pin_mask=None) -> (f', n_flips)
        One round.  Edge (a, b) = (min, max) of face count 2 whose sides run in opposite directions: one face holds a -> b, its third vertex is c;
        the other holds b -> a, its third vertex is d.  It is a candidate when c != d, no edge (c, d) exists, gain > 0 with
        gain = sum |val - tgt| over a, b, c, d minus the same sum with val(a), val(b) one lower and val(c), val(d) one higher (tgt = 4 for a pinned
        vertex, else 6), n1 = nrm(a, b, c) and n2 = nrm(b, a, d) pass the cosine test at c2 = 0.75 (30 degrees, the script's crease angle: features
        are not flipped), and m1 = nrm(a, d, c), m2 = nrm(d, b, c) each pass it at c2 = 0.25 against n1 and n2.
        key = (15 - min(gain, 15)) << 32 | rank; claim set a, b, c, d.  A selected edge flips in place: the face that held a -> b becomes the row
        (a, d, c), the other the row (d, b, c); face order, face count and parents stay.  Up to `rounds` rounds; one without a flip ends the loop.
    smooth_tangential(v, faces, pin_mask=None) -> v'
        One Jacobi pass (old positions read, new ones written).  A vertex p that is not pinned and has a neighbour: g = (the sum of its neighbours,
        from 0, in ascending index) * (1.0f / deg); n = the sum of nrm of its faces, from 0, in ascending face index, each component divided by
        sqrt(dot(n, n)) (a zero sum: the vertex stays); d = g - p, t = dot(n, d), p' = (p + d) - n * t.  The move is rejected, and the vertex stays,
        when a face of it would get dot(nrm with p', nrm) <= 0.  That test damps fold-overs; it is no guarantee against them (two neighbours
        that move in the same pass are not seen together).
    isotropic_remesh(v, faces, target_len, iterations=3, collapse_rounds=8, flip_rounds=8, reproject=True, pin_mask=None, accel_bvh=None)
            -> (v', f', parent)
        Per iteration: refine_long_edges(4/3 target_len, iterations=1); collapse_short_edges(lo = 4/5 target_len, hi = 4/3 target_len,
        collapse_rounds); flip_edges(flip_rounds); smooth_tangential; with `reproject`, every vertex that moved in the iteration (a new midpoint, a
        collapse survivor whose position changed, a smoothed vertex) goes to (b0 A + b1 B) + b2 C, raytrace.Bvh.nearest's closest point on the
        INPUT surface (one Bvh of the input per call, or the caller's accel_bvh of that same input; tri == -1 leaves the vertex).  A pin_mask follows the
        vertices through the splits (new midpoints are not pinned) and through vmap.  (The 4/3 and 4/5 products are formed in double precision
        and rounded to float32 once.)"""
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


# ---- collapse, flip, smooth, reproject (csrc/meshremesh.hip) --------------------------------------------------------------------------------

def _check(what, v, faces, pin_mask):
    f = _mt._faces(faces, what)
    if v.dim() != 2 or v.shape[1] != 3 or v.dtype != torch.float32:
        raise RuntimeError(f'{what}: expected positions [n,3] float32, got {tuple(v.shape)} {v.dtype}')
    n = int(v.shape[0])
    if pin_mask is not None and (pin_mask.shape != (n,) or pin_mask.dtype not in (torch.bool, torch.uint8)):
        raise RuntimeError(f'{what}: expected pin_mask [{n}] bool or uint8, got {tuple(pin_mask.shape)} {pin_mask.dtype}')
    if f.shape[0] and (n == 0 or int(f.min()) < 0 or int(f.max()) >= n):
        raise RuntimeError(f'{what}: a face index outside [0, nv)')
    return v.detach().contiguous(), f, None if pin_mask is None else pin_mask.bool()


class _Adjacency:
    """what the kernels of csrc/meshremesh.hip walk (module docstring, "adjacency" and "pinned"), of faces [F,3] with every index in [0, n)"""

    def __init__(self, f, n, pin):
        dev = f.device
        fl = f.long()
        a, b = fl.reshape(-1), fl[:, [1, 2, 0]].reshape(-1)
        keys, cnt = torch.unique((torch.minimum(a, b) << 32) | torch.maximum(a, b), return_counts=True)        # ascending
        elo, ehi = keys >> 32, keys & 0xffffffff
        pinned = torch.zeros(n, dtype=torch.bool, device=dev) if pin is None else pin.clone()
        odd = cnt != 2
        pinned[elo[odd]] = True
        pinned[ehi[odd]] = True
        proper = elo != ehi
        nk = torch.sort(torch.cat([(elo[proper] << 32) | ehi[proper], (ehi[proper] << 32) | elo[proper]])).values
        fk = torch.unique((a << 32) | torch.arange(f.shape[0], device=dev).repeat_interleave(3))
        zero = torch.zeros(1, dtype=torch.long, device=dev)
        self.n, self.ne, self.nnbr, self.nvf = n, int(keys.shape[0]), int(nk.shape[0]), int(fk.shape[0])
        self.elo, self.ehi, self.ecnt = elo.int().contiguous(), ehi.int().contiguous(), cnt.int().contiguous()
        self.noffs = torch.cat([zero, torch.cumsum(torch.bincount(nk >> 32, minlength=n), 0)]).int().contiguous()
        self.nbr = (nk & 0xffffffff).int().contiguous()
        self.foffs = torch.cat([zero, torch.cumsum(torch.bincount(fk >> 32, minlength=n), 0)]).int().contiguous()
        self.vf = (fk & 0xffffffff).int().contiguous()
        self.pinned = pinned.to(torch.uint8).contiguous()


def _collapse_round(v, f, lo, hi, pin):
    """-> None when nothing collapsed, else (v', f', parent, vmap, keep): keep [n] bool = the vertices that stay"""
    dev = v.device
    n, nf = int(v.shape[0]), int(f.shape[0])
    idx64 = f.dtype == torch.int64
    A = _Adjacency(f, n, pin)
    ekey = torch.empty(A.ne, dtype=torch.int64, device=dev)
    claim = torch.empty(n, dtype=torch.int64, device=dev)
    counts = torch.zeros(4, dtype=torch.int32, device=dev)
    L.call('remesh_collapse_claim', v, f, idx64, nf, n, A.elo, A.ehi, A.ecnt, A.ne, A.noffs, A.nbr, A.nnbr, A.foffs, A.vf, A.nvf, A.pinned, lo, hi, ekey, claim, counts)
    vout = v.clone()
    ident = torch.arange(n, dtype=torch.int32, device=dev)
    remap = ident.clone()
    fdrop = torch.zeros(nf, dtype=torch.uint8, device=dev)
    L.call('remesh_collapse_select', v, f, idx64, nf, n, A.elo, A.ehi, A.ne, A.noffs, A.nbr, A.nnbr, A.foffs, A.vf, A.nvf, A.pinned, ekey, claim, vout, remap,
           fdrop, counts)
    nc, nd, word, _ = counts.tolist()                                               # the round's one read-back
    _mt._raise(word, 'collapse_short_edges')
    if nc == 0:
        return None
    keep = remap == ident
    newidx = (torch.cumsum(keep, 0) - 1).int().contiguous()
    kf = (fdrop == 0).long()
    offs = (torch.cumsum(kf, 0) - kf).contiguous()
    nout = nf - nd
    fout = torch.empty(nout, 3, dtype=f.dtype, device=dev)
    parent = torch.empty(nout, dtype=torch.int32, device=dev)
    L.call('remesh_collapse_faces', f, idx64, nf, n, remap, newidx, fdrop, offs, nout, fout, parent)
    return vout[keep].contiguous(), fout, parent.long(), newidx[remap.long()].long(), keep


def _collapse(v, f, lo, hi, rounds, pin):
    """-> (v', f', parent, vmap, pin', src): src int64 [n'] = the input row each output vertex was"""
    dev = v.device
    parent = torch.arange(f.shape[0], dtype=torch.int64, device=dev)
    vmap = torch.arange(v.shape[0], dtype=torch.int64, device=dev)
    src = vmap
    for _ in range(int(rounds)):
        if f.shape[0] == 0:
            break
        r = _collapse_round(v, f, lo, hi, pin)
        if r is None:
            break
        v, f, p, m, keep = r
        parent, vmap, src = parent[p], m[vmap], src[keep]
        if pin is not None:
            pin = pin[keep]
    return v, f, parent, vmap, pin, src


def _lengths(what, **kw):
    out = []
    for k, x in kw.items():
        x = float(x)
        if not x > 0.0:
            raise RuntimeError(f'{what}: {k} must be > 0, got {x}')
        out.append(x)
    return out


def collapse_short_edges(v, faces, lo, hi, rounds=8, pin_mask=None):
    v, f, pin = _check('collapse_short_edges', v, faces, pin_mask)
    lo, hi = _lengths('collapse_short_edges', lo=lo, hi=hi)
    return _collapse(v, f, lo, hi, rounds, pin)[:4]


def _flip(v, f, rounds, pin):
    dev = v.device
    n, nf = int(v.shape[0]), int(f.shape[0])
    idx64 = f.dtype == torch.int64
    f = f.clone()
    total = 0
    for _ in range(int(rounds)):
        if nf == 0:
            break
        A = _Adjacency(f, n, pin)
        ekey = torch.empty(A.ne, dtype=torch.int64, device=dev)
        equad = torch.empty(A.ne, 4, dtype=torch.int32, device=dev)
        claim = torch.empty(n, dtype=torch.int64, device=dev)
        counts = torch.zeros(4, dtype=torch.int32, device=dev)
        L.call('remesh_flip_claim', v, f, idx64, nf, n, A.elo, A.ehi, A.ecnt, A.ne, A.noffs, A.nbr, A.nnbr, A.foffs, A.vf, A.nvf, A.pinned, ekey, equad, claim, counts)
        L.call('remesh_flip_apply', f, idx64, nf, n, A.elo, A.ehi, A.ne, ekey, equad, claim, counts)
        done, _, word, _ = counts.tolist()                                          # the round's one read-back
        _mt._raise(word, 'flip_edges')
        if done == 0:
            break
        total += done
    return f, total


def flip_edges(v, faces, rounds=8, pin_mask=None):
    v, f, pin = _check('flip_edges', v, faces, pin_mask)
    return _flip(v, f, rounds, pin)


def _smooth(v, f, pin):
    n, nf = int(v.shape[0]), int(f.shape[0])
    if n == 0 or nf == 0:
        return v.clone()
    A = _Adjacency(f, n, pin)
    out = torch.empty_like(v)
    L.call('remesh_smooth', v, f, f.dtype == torch.int64, nf, n, A.noffs, A.nbr, A.nnbr, A.foffs, A.vf, A.nvf, A.pinned, out)
    return out


def smooth_tangential(v, faces, pin_mask=None):
    v, f, pin = _check('smooth_tangential', v, faces, pin_mask)
    return _smooth(v, f, pin)


def _reproject(v, at, bvh, v0, f0):
    """v with the rows `at` (int64) moved to their closest point on the mesh (v0, f0 int64) that `bvh` holds: (b0 A + b1 B) + b2 C"""
    if at.numel() == 0:
        return v
    near = bvh.nearest(v[at])
    tri, b = near.tri.long().clamp_min(0), near.bary
    A, B, C = v0[f0[tri, 0]], v0[f0[tri, 1]], v0[f0[tri, 2]]
    pnt = (b[:, 0:1] * A + b[:, 1:2] * B) + b[:, 2:3] * C
    out = v.clone()
    out[at] = torch.where((near.tri >= 0)[:, None], pnt, v[at])
    return out


def isotropic_remesh(v, faces, target_len, iterations=3, collapse_rounds=8, flip_rounds=8, reproject=True, pin_mask=None, accel_bvh=None):
    v, f, pin = _check('isotropic_remesh', v, faces, pin_mask)
    t, = _lengths('isotropic_remesh', target_len=target_len)
    dev = v.device
    parent = torch.arange(f.shape[0], dtype=torch.int64, device=dev)
    if f.shape[0] == 0:
        return v, f, parent
    hi, lo = t * 4.0 / 3.0, t * 4.0 / 5.0
    v0, f0, bvh = v, f.long(), accel_bvh
    if reproject and bvh is None:
        from . import raytrace as _rt
        bvh = _rt.Bvh(v0, f)
    for _ in range(int(iterations)):
        n = v.shape[0]
        v, f, p = refine_long_edges(v, f, hi, iterations=1)
        parent = parent[p]
        extra = v.shape[0] - n
        moved = torch.zeros(v.shape[0], dtype=torch.bool, device=dev)
        moved[n:] = True
        if pin is not None and extra:
            pin = torch.cat([pin, torch.zeros(extra, dtype=torch.bool, device=dev)])
        vc, f, p, vmap, pin, src = _collapse(v, f, lo, hi, collapse_rounds, pin)
        parent = parent[p]
        carried = torch.zeros(vc.shape[0], dtype=torch.long, device=dev).index_add_(0, vmap, moved.long())      # a survivor inherits the mark of the end it absorbed
        moved = (carried > 0) | (vc != v[src]).any(1)
        f, _ = _flip(vc, f, flip_rounds, pin)
        v = _smooth(vc, f, pin)
        moved |= (v != vc).any(1)
        if reproject:
            v = _reproject(v, torch.nonzero(moved).reshape(-1), bvh, v0, f0)
    return v, f, parent
