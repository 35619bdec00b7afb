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
        and rounded to float32 once.)

Quadric decimation (csrc/meshdecim.hip) for the level-of-detail export (d3h.export.lod_chain): the shape-keeping way to fewer faces, where
collapse_short_edges is the uniform-length step of remeshing.  Conventions as above (adjacency, selection, validation) except where stated.

    decimate(v, faces, target_faces, rounds=256, window=3.0, min_window=256, boundary='slide', max_cost=inf, pin_mask=None)
            -> (v', f', parent, vmap, info)
        v', f', parent, vmap as for collapse_short_edges.  info = {'rounds': rounds that collapsed something, 'collapses': their collapses,
        'reached': F' <= target_faces + 1 (a collapse of an interior edge takes two faces, so an odd distance stops one short), 'max_cost': the
        largest float64 cost taken (0.0 when nothing collapsed)}.  F <= target_faces returns the input.  F' >= target_faces always.
        arithmetic    quadrics, placement and cost in float64 (positions promoted from float32), every operation rounded once in the order
                      written, no contraction, dot / cross / len2 as above and
                        det3(m) = (m00 (m11 m22 - m12 m21) - m01 (m10 m22 - m12 m20)) + m02 (m10 m21 - m11 m20)
                        E(Q, q): r = ((a00 x + a01 y) + a02 z, (a01 x + a11 y) + a12 z, (a02 x + a12 y) + a22 z);
                                 e = (((x rx + y ry) + z rz) + 2 ((b0 x + b1 y) + b2 z)) + c;  e < 0 gives 0
                      for a quadric Q = (a00, a01, a02, b0, a11, a12, b1, a22, b2, c) and q = (x, y, z), a float32 point promoted.  The normal
                      test is the float32 cosine test above at c2 = 0.04f (cos >= 0.2).
        quadrics      built ONCE, from the input mesh, one thread per vertex as a gather (no float atomics): Q[i] = the sum from 0, over the faces
                      of i in ascending index, of w (ux ux, ux uy, ux uz, ux d, uy uy, uy uz, uy d, uz uz, uz d, d d) -- each product formed, then
                      times w -- with n = cross(p1 - p0, p2 - p0) of the face's rows, l = sqrt(dot(n, n)), u = n / l, d = -dot(u, p0), w = l * 0.5
                      (l == 0, or not l > 0: the face adds nothing).  With boundary='slide' every edge (a, b) = (min, max) of face count 1 then
                      adds, to both ends, in ascending edge rank, the plane through the edge perpendicular to its face (the first face of the
                      vertex, in ascending index, that holds the other end; none if that face has l == 0): e = p[b] - p[a], m = cross(e, u),
                      lm = sqrt(dot(m, m)) (0: nothing), m / lm in the place of u, d = -dot(m / lm, p[a]), w = 4 dot(e, e) (the 4 is
                      DC_BOUNDARY_WEIGHT of the source).  Quadrics travel with the vertices: a collapse leaves Q[a] + Q[b] (a = min first) on its
                      survivor; nothing is recomputed from the reduced mesh.
        classes       per round, from the faces as they stand.  Pinned: on an edge of face count > 2, on an edge with min == max, on a number of
                      edges of face count 1 other than 0 or 2, or set in pin_mask (which follows the vertices); with boundary='pin' every
                      vertex on an edge of face count 1.  Boundary: on exactly two edges of face count 1, not pinned.  Interior: the rest.  Pinned
                      vertices come back bit-unchanged and never disappear; boundary vertices thin out and never move.
        candidates    edge (a, b) = (min, max), a != b, Qe = Q[a] + Q[b], of one of three kinds:
                        face count 2, both ends interior: A = Qe's 3 x 3 part, det = det3(A), t = (a00 + a11) + a22, x = the solution of
                          A x = -b by Cramer's rule (det3 with column k replaced, divided by det), mid = (v[a] + v[b]) * 0.5 in float64.  x is
                          ACCEPTED when |det| > 1e-9 ((t t) t), x is finite and len2(x, mid) <= 4 len2(v[a], v[b]).  q = of x (if accepted), mid,
                          v[a], v[b], each rounded to float32, the one of smallest E(Qe, q), a tie to the earlier in that list; survivor a
                        face count 2, exactly one end interior: the other end survives where it is, q = its position (both ends boundary or
                          pinned: a chord, no candidate)
                        face count 1, boundary='slide', both ends boundary: q = v[b] if E(Qe, v[b]) < E(Qe, v[a]) else v[a]; that end survives
                      with cost = E(Qe, q) finite and <= max_cost (a NaN or infinite cost is no candidate), and these checks on the round's
                      input, before any claim (for the reason given under collapse_short_edges):
                        link    N(a) and N(b) share exactly two vertices, each of valence > 3 (face count 2), or exactly one, of valence > 2
                                (face count 1)
                        normal  every face that holds a or b but not both passes the cosine test at c2 = 0.04f between nrm of its rows and nrm
                                of its rows with that end replaced by q (a face of zero area fails it and so holds its corners in place)
        window        need = ceil((F - target_faces) / 2), W = max(ceil(window * need), min_window).  Only the W candidates of smallest
                      bits(float32(cost)) << 32 | rank place claims; the threshold is the W-th entry of a device sort, handed to the kernel as a
                      device value (no read-back)
        selection     key = (bits(float32(cost)) >> 20) << 32 | mix(rank, round) -- the cost's exponent and top three mantissa bits, ties
                      broken by mix(rank, round): x = rank ^ (round * 0x9e3779b9); x ^= x >> 16; x *= 0x85ebca6b; x ^= x >> 13; x *= 0xc2b2ae35;
                      x ^= x >> 16 (32-bit, a bijection of the rank; round counts from 0) -- with the rank as tie-break a run of equal costs
                      along the mesh yields one winner per round.  Claim set {a, b} + N(a) + N(b)
        trim          the selected keys ascending; the longest prefix whose dropped faces (the edge's face count each) sum to at most
                      F - target_faces collapses (a device scan, the cut handed to the kernel as a device value)
        loop          ends when F' <= target_faces, when a round collapses nothing, or after `rounds` rounds; one read-back per round (collapses,
                      dropped faces, error word, largest cost, together) and one for the quadrics' error word before the first.  Sizes
                      (profiles/decimate_probe.md): a closed-neighbourhood claim lets a round take one to three percent of the edges, so 1/4
                      of the faces takes about 50 to 140 rounds and 1/16 about 80 to 240, which is what rounds = 256 is for; min_window keeps
                      the tail from starving when `need` gets small"""
import math
import struct

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


# ---- quadric decimation (csrc/meshdecim.hip) ---------------------------------------------------------------------------------------------------

class _DecimAdjacency(_Adjacency):
    """_Adjacency plus what decimation reads (module docstring, "classes"): ncnt [nnbr] int32, the face count of the edge to each neighbour, and
    vclass [n] uint8, 0 interior / 1 boundary / 2 pinned"""

    def __init__(self, f, n, pin, slide):
        super().__init__(f, n, None)
        dev = f.device
        elo, ehi, cnt = self.elo.long(), self.ehi.long(), self.ecnt.long()
        own = torch.repeat_interleave(torch.arange(n, device=dev), (self.noffs[1:] - self.noffs[:-1]).long())
        other = self.nbr.long()
        rank = torch.searchsorted((elo << 32) | ehi, (torch.minimum(own, other) << 32) | torch.maximum(own, other))
        self.ncnt = self.ecnt[rank].contiguous()
        pinned = torch.zeros(n, dtype=torch.bool, device=dev) if pin is None else pin.clone()
        fixed = (cnt > 2) | (elo == ehi)
        pinned[elo[fixed]] = True
        pinned[ehi[fixed]] = True
        open_ = (cnt == 1) & (elo != ehi)
        nopen = torch.bincount(torch.cat([elo[open_], ehi[open_]]), minlength=n)
        pinned |= (nopen != 0) & (nopen != 2) if slide else nopen != 0
        self.vclass = torch.where(pinned, 2, torch.where(nopen == 2, 1, 0)).to(torch.uint8).contiguous()


def _decimate_round(v, f, Q, pin, target, window, min_window, slide, max_cost, rnd):
    """-> None when nothing collapsed, else (v', f', parent, vmap, keep, Q', collapses, largest cost)"""
    dev = v.device
    n, nf = int(v.shape[0]), int(f.shape[0])
    idx64 = f.dtype == torch.int64
    A = _DecimAdjacency(f, n, pin, slide)
    ne = A.ne
    wkey, ekey, skey = (torch.empty(ne, dtype=torch.int64, device=dev) for _ in range(3))
    eq = torch.empty(ne, 3, dtype=torch.float32, device=dev)
    esurv = torch.empty(ne, dtype=torch.int32, device=dev)
    ecost = torch.empty(ne, dtype=torch.float64, device=dev)
    claim = torch.empty(n, dtype=torch.int64, device=dev)
    counts = torch.zeros(4, dtype=torch.int32, device=dev)
    maxcost = torch.zeros(1, dtype=torch.int64, device=dev)
    L.call('decim_cost', v, f, idx64, nf, n, A.elo, A.ehi, A.ecnt, ne, A.noffs, A.nbr, A.nnbr, A.foffs, A.vf, A.nvf, A.vclass, Q, max_cost, slide, rnd, wkey, ekey,
           eq, esurv, ecost, counts)
    need = (nf - target + 1) // 2
    w = min(max(int(math.ceil(window * need)), min_window), ne)
    wthr = torch.sort(wkey).values[w - 1:w].contiguous()                           # the window's threshold stays on the device
    L.call('decim_claim', A.elo, A.ehi, ne, n, A.noffs, A.nbr, A.nnbr, wkey, wthr, ekey, claim)
    L.call('decim_select', A.elo, A.ehi, ne, n, A.noffs, A.nbr, A.nnbr, ekey, claim, skey)
    sk, order = torch.sort(skey)                                                   # the trim: selected keys ascending, the prefix that stays above the target
    chosen = sk != _MAXKEY
    fits = chosen & (torch.cumsum(torch.where(chosen, A.ecnt[order].long(), 0), 0) <= nf - target)
    cut = torch.cat([sk, sk.new_full((1,), _MAXKEY)])[fits.sum().reshape(1)].contiguous()
    vout, qout = v.clone(), Q.clone()
    ident = torch.arange(n, dtype=torch.int32, device=dev)
    remap = ident.clone()
    fdrop = torch.zeros(nf, dtype=torch.uint8, device=dev)
    L.call('decim_apply', f, idx64, nf, n, A.elo, A.ehi, ne, A.foffs, A.vf, A.nvf, Q, skey, cut, eq, esurv, ecost, vout, qout, remap, fdrop, counts, maxcost)
    nc, nd, word, _, bits = torch.cat([counts.long(), maxcost]).tolist()           # the round's one read-back
    _mt._raise(word, 'decimate')
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
    return (vout[keep].contiguous(), fout, parent.long(), newidx[remap.long()].long(), keep, qout[keep].contiguous(), nc,
            struct.unpack('<d', struct.pack('<q', bits))[0])


def _quadrics(v, f, slide):
    """Q [n,10] float64 of the mesh (module docstring, "quadrics")"""
    n, nf = int(v.shape[0]), int(f.shape[0])
    A = _DecimAdjacency(f, n, None, slide)
    Q = torch.empty(n, 10, dtype=torch.float64, device=v.device)
    counts = torch.zeros(4, dtype=torch.int32, device=v.device)
    L.call('decim_quadrics', v, f, f.dtype == torch.int64, nf, n, A.noffs, A.nbr, A.ncnt, A.nnbr, A.foffs, A.vf, A.nvf, slide, Q, counts)
    return Q, counts


def decimate(v, faces, target_faces, rounds=256, window=3.0, min_window=256, boundary='slide', max_cost=float('inf'), pin_mask=None):
    v, f, pin = _check('decimate', v, faces, pin_mask)
    target, rounds, window, min_window, max_cost = int(target_faces), int(rounds), float(window), int(min_window), float(max_cost)
    if target < 0:
        raise RuntimeError(f'decimate: target_faces must be >= 0, got {target_faces}')
    if not window > 0.0 or min_window < 1:
        raise RuntimeError(f'decimate: window must be > 0 and min_window >= 1, got {window}, {min_window}')
    if boundary not in ('slide', 'pin'):
        raise RuntimeError(f"decimate: boundary must be 'slide' or 'pin', got {boundary!r}")
    if not max_cost >= 0.0 or rounds < 0:
        raise RuntimeError(f'decimate: max_cost and rounds must be >= 0, got {max_cost}, {rounds}')
    dev = v.device
    slide = boundary == 'slide'
    parent = torch.arange(f.shape[0], dtype=torch.int64, device=dev)
    vmap = torch.arange(v.shape[0], dtype=torch.int64, device=dev)
    info = {'rounds': 0, 'collapses': 0, 'reached': True, 'max_cost': 0.0}
    if f.shape[0] <= target:
        return v, f, parent, vmap, info
    Q, counts = _quadrics(v, f, slide)
    _mt._raise(int(counts[2]), 'decimate')                                         # once per call, before the rounds
    for rnd in range(rounds):
        if f.shape[0] <= target:
            break
        r = _decimate_round(v, f, Q, pin, target, window, min_window, slide, max_cost, rnd)
        if r is None:
            break
        v, f, p, m, keep, Q, nc, cost = r
        parent, vmap = parent[p], m[vmap]
        if pin is not None:
            pin = pin[keep]
        info['rounds'] += 1
        info['collapses'] += nc
        info['max_cost'] = max(info['max_cost'], cost)
    info['reached'] = int(f.shape[0]) <= target + 1
    return v, f, parent, vmap, info
