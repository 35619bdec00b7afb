"""Check functions of the distance queries on the BVH (csrc/bvhdist.hip, d3h/raytrace.py: Bvh.nearest / winding / signed_distance) and of their opt-in
wiring (meshops.mesh_wsdf(accel=), watertight, the hand-off's garment field), shared by tests/test_bvhdist_emul.py (host emulation of the kernel
sources) and tests/test_gpu_bvhdist.py (MI355X).  Same shapes on both.  Every mesh and query set is generated here from a seed.

Meshes: the occlusion meshes of tests/optixutils_cases.py, a planar fan (every triangle in z = 0.25: flat boxes), soup64 with every triangle stored twice
(index F + i repeats i), a closed icosphere(2) of 320 faces and the same with the faces above z = 0.6 r removed.
Queries: 1000 per mesh (15 waves and 40 lanes): 950 uniform in 1.5 x the bounding box, 50 at distance 10^3.  An axis along which the box has no extent
(the fan's z) takes the largest extent instead: IN the plane of a triangle its solid angle is +- half a turn by the sign of a zero, in any precision.

Yardsticks, all numpy, each run in float64 and again in float32 for the project's PARITY RULE (optixutils_cases.assert_close: max|got - f64| / max|f64|
<= max(5 x the float32 yardstick's own error, 2^-20) per tensor):
  nearest   closest point by Ericson's region test over ALL triangles whose cross product is not exactly zero
  moments   sums over the leaves below every node of the read-back tree
  winding   (a) the float64 sum of van Oosterom-Strackee solid angles over all triangles; (b) a host walk of the read-back tree (nodes, moments) with
            the kernel's accept rule, |c - q|^2 > (beta r)^2; a query for which any visited node lies within 1e-5 relative of that equality is left out
            (at most 1 %, asserted before the kernel runs)
Every figure is printed before it is asserted (run with -s)."""
import functools
import math

import numpy as np
import pytest
import torch

import handoff_cases as HC
import optixutils_cases as OC
from d3h import _lib as L
from d3h import meshops as MO
from d3h import raytrace as RT

FLOOR = OC.FLOOR
assert_close = OC.assert_close
MESHES = OC.MESHES + ('fan', 'soup64x2', 'ico', 'ico_open')
NO_ZERO_AREA = tuple(m for m in MESHES if m not in ('zero_area', 'soup0'))
N_Q = 1000
N_FAR = 50
ICO_C, ICO_R = np.array([0.1, -0.05, 0.2]), 0.8
BETAS = (2.0, 3.0, 4.0)


def _icosphere(level):
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(x, np.float64) / np.linalg.norm(x) for x in v]
    for _ in range(level):
        mid, g = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                x = v[a] + v[b]
                v.append(x / np.linalg.norm(x))
                mid[k] = len(v) - 1
            return mid[k]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            g += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = g
    v, f = np.array(v), np.array(f, np.int32)
    assert HC._signed_volume(v, f) > 0                       # wound outward
    return v, f


@functools.lru_cache(maxsize=None)
def mesh(name):
    """-> (verts float32 [V,3], tris int32 / int64 [F,3])"""
    if name in OC.MESHES:
        return OC.mesh(name)
    rng = OC._rng('bvhdist mesh ' + name)
    if name == 'fan':
        k = 24
        ang = np.sort(rng.uniform(0.0, 2.0 * np.pi, k))
        rad = rng.uniform(0.5, 1.0, k)
        rim = np.stack([0.1 + rad * np.cos(ang), -0.2 + rad * np.sin(ang), np.full(k, 0.25)], 1)
        v = np.concatenate([[[0.1, -0.2, 0.25]], rim]).astype(np.float32)
        i = np.arange(k)
        return v, np.stack([np.zeros(k, np.int64), 1 + i, 1 + (i + 1) % k], 1).astype(np.int32)
    if name == 'soup64x2':
        v, f = OC.mesh('soup64')
        return v, np.concatenate([f, f])
    if name in ('ico', 'ico_open'):
        v, f = _icosphere(2)
        assert len(f) == 320
        if name == 'ico_open':
            f = f[v[f].mean(1)[:, 2] <= 0.6]
            assert 200 < len(f) < 320
        return (ICO_C + ICO_R * v).astype(np.float32), f
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def queries(name):
    v, f = mesh(name)
    rng = OC._rng('bvhdist queries ' + name)
    used = v[np.unique(f.astype(np.int64))] if len(f) and len(v) else np.array([[-1.0, -1, -1], [1, 1, 1]])
    lo, hi = used.min(0).astype(np.float64), used.max(0).astype(np.float64)
    c, half = 0.5 * (lo + hi), 0.75 * (hi - lo)
    half = np.where(half > 0, half, half.max() if half.max() > 0 else 1.0)
    q = c + rng.uniform(-1.0, 1.0, (N_Q, 3)) * half
    d = rng.standard_normal((N_FAR, 3))
    q[N_Q - N_FAR:] = c + 1.0e3 * d / np.linalg.norm(d, axis=1, keepdims=True)
    return q.astype(np.float32)


def live_triangles(v, f):
    """indices of the triangles whose cross product is not exactly zero (optixutils_cases.brute's rule)"""
    if len(f) == 0 or len(v) == 0:
        return np.zeros(0, np.int64)
    t = v.astype(np.float64)[f.astype(np.int64)]
    n = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    return np.nonzero((n * n).sum(1) > 0)[0]


def dist_matrix(q, v, f, dt):
    """[N, F'] distances of the queries to the live triangles, computed in dt"""
    live = live_triangles(v, f)
    t = v.astype(dt)[f[live].astype(np.int64)]
    out = [np.sqrt(HC._tri_dist2(q[s:s + 256].astype(dt)[:, None], t[None, :, 0], t[None, :, 1], t[None, :, 2])) for s in range(0, len(q), 256)]
    return np.concatenate(out), live


def solid_angles(q, A, B, C):
    """van Oosterom-Strackee, radians, [N, F] in the arrays' type"""
    sq = lambda x: HC._dot(x, x)
    ra, rb, rc = A - q, B - q, C - q
    la, lb, lc = np.sqrt(sq(ra)), np.sqrt(sq(rb)), np.sqrt(sq(rc))
    det = HC._dot(ra, np.cross(rb, rc))
    den = la * lb * lc + HC._dot(ra, rb) * lc + HC._dot(ra, rc) * lb + HC._dot(rb, rc) * la
    return q.dtype.type(2) * np.arctan2(det, den)


def winding_sum(q, v, f, dt):
    """w in turns [N]: the sum over all live triangles, in dt"""
    live = live_triangles(v, f)
    if len(live) == 0:
        return np.zeros(len(q))
    t = v.astype(dt)[f[live].astype(np.int64)]
    out = [solid_angles(q[s:s + 256].astype(dt)[:, None], t[None, :, 0], t[None, :, 1], t[None, :, 2]).sum(1, dtype=dt) for s in range(0, len(q), 256)]
    return (np.concatenate(out) / dt(4 * np.pi)).astype(np.float64)


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> dict: q, the float64 / float32 distance matrices' minima, the float64 matrix itself, live indices, w64 / w32 (exact sums)"""
    v, f = mesh(name)
    q = queries(name)
    live = live_triangles(v, f)
    if len(live) == 0:
        return dict(q=q, live=live, D=np.zeros((N_Q, 0)), d64=np.full(N_Q, np.inf), d32=np.full(N_Q, np.inf), w64=np.zeros(N_Q), w32=np.zeros(N_Q))
    D, _ = dist_matrix(q, v, f, np.float64)
    D32, _ = dist_matrix(q, v, f, np.float32)
    return dict(q=q, live=live, D=D, d64=D.min(1), d32=D32.min(1).astype(np.float64), w64=winding_sum(q, v, f, np.float64), w32=winding_sum(q, v, f, np.float32))


def T(dev, a):
    return torch.as_tensor(a, device=dev)


def build(dev, name):
    v, f = mesh(name)
    return RT.Bvh(T(dev, v), T(dev, f))


# ---- nearest triangle -----------------------------------------------------------------------------------------------------------------------------
def check_nearest(dev, name):
    """checks 1, 2, 3 and 6 of the nearest query: the distance, the returned triangle, the barycentrics; never a zero-area triangle"""
    v, f = mesh(name)
    ref = reference(name)
    q, live = ref['q'], ref['live']
    d2, tri, bary = build(dev, name).nearest(T(dev, q))
    assert d2.dtype == torch.float32 and tri.dtype == torch.int32 and bary.dtype == torch.float32
    assert tuple(d2.shape) == (N_Q,) and tuple(tri.shape) == (N_Q,) and tuple(bary.shape) == (N_Q, 3)
    d2, tri, bary = d2.cpu().numpy(), tri.cpu().numpy(), bary.cpu().numpy()
    if len(live) == 0:
        assert np.all(np.isposinf(d2)) and np.all(tri == -1) and np.all(bary == 0)
        return
    assert_close(f'{name}: sqrt(d2) against the float64 loop', np.sqrt(d2), ref['d64'], ref['d32'])
    col = np.full(len(f), -1)
    col[live] = np.arange(len(live))
    assert np.all(tri >= 0) and np.all(tri < len(f)) and np.all(col[tri] >= 0), 'an index out of range, or a zero-area triangle'
    assert_close(f'{name}: float64 distance to the returned triangle', ref['D'][np.arange(N_Q), col[tri]], ref['d64'], ref['d32'])
    s = bary.astype(np.float64).sum(1)
    print(f'{name}: min bary {bary.min():.3e}, max |sum - 1| {np.abs(s - 1).max():.3e}')
    assert bary.min() >= 0 and np.abs(s - 1).max() <= FLOOR
    cp = (bary.astype(np.float64)[:, :, None] * v.astype(np.float64)[f[tri].astype(np.int64)]).sum(1)
    assert_close(f'{name}: |p - sum bary v| against the float64 loop', np.linalg.norm(q.astype(np.float64) - cp, axis=1), ref['d64'], ref['d32'])


def check_nearest_ties(dev):
    """check 4: duplicated triangles never return the copy; a query ON a shared vertex returns d2 = 0 and the smallest incident index"""
    v, f = mesh('soup64x2')
    tri = build(dev, 'soup64x2').nearest(T(dev, queries('soup64x2'))).tri.cpu().numpy()
    print(f'soup64x2: max tri {tri.max()} of F / 2 = {len(f) // 2}')
    assert np.all(tri >= 0) and np.all(tri < len(f) // 2)
    v, f = mesh('int64')
    used = np.unique(f)
    d2, tri, bary = build(dev, 'int64').nearest(T(dev, v[used]))
    want = np.array([np.nonzero((f == u).any(1))[0].min() for u in used])
    shared = np.array([(f == u).any(1).sum() for u in used])
    print(f'int64: {len(used)} vertex queries, {int((shared > 1).sum())} on shared vertices; max d2 {float(d2.max()):.1e}')
    assert (shared > 1).sum() > 20
    assert np.all(d2.cpu().numpy() == 0)
    assert np.array_equal(tri.cpu().numpy(), want)


def check_nearest_bits(dev, name, exact):
    """check 5: sqrt(d2) against |mesh_wsdf|, the brute-force minimum of the same arithmetic.  Bit equality is the test of the conservative skip; it is
    asserted where both kernels round alike by construction (`exact`: the emulation, compiled without contraction), printed elsewhere."""
    v, f = mesh(name)
    q = T(dev, queries(name))
    got = np.sqrt(build(dev, name).nearest(q).d2.cpu().numpy())              # numpy's square root is correctly rounded, as the kernels' is
    brute = MO.mesh_wsdf(q, T(dev, v), T(dev, f.astype(np.int32)), want_w=False)[0].abs().cpu().numpy()
    diff = int((got.view(np.uint32) != brute.view(np.uint32)).sum())
    print(f'{name}: {diff} of {N_Q} distances differ in their bits from the brute-force minimum')
    if exact:
        assert diff == 0
    else:
        ref = reference(name)
        assert_close(f'{name}: sqrt(d2) against the float64 loop', got, ref['d64'], ref['d32'])


def check_nearest_edges(dev):
    """check 7 and the batch shapes: F = 0, V = 0, non-finite queries, n = 1, n = 0, leading dimensions"""
    empty = build(dev, 'soup0')
    r = empty.nearest(torch.zeros(5, 3, device=dev))
    assert np.all(np.isposinf(r.d2.cpu().numpy())) and np.all(r.tri.cpu().numpy() == -1) and np.all(r.bary.cpu().numpy() == 0)
    assert np.all(empty.winding(torch.zeros(5, 3, device=dev)).cpu().numpy() == 0)
    assert np.all(np.isposinf(empty.signed_distance(torch.zeros(5, 3, device=dev)).cpu().numpy()))
    bvh = build(dev, 'soup65')
    q = queries('soup65')[:6].copy()
    q[1, 0], q[3, 2], q[4, 1] = np.nan, np.inf, -np.inf
    r = bvh.nearest(T(dev, q))
    bad = np.array([False, True, False, True, True, False])
    d2, tri, bary = r.d2.cpu().numpy(), r.tri.cpu().numpy(), r.bary.cpu().numpy()
    assert np.all(np.isposinf(d2[bad])) and np.all(tri[bad] == -1) and np.all(bary[bad] == 0)
    assert np.all(np.isfinite(d2[~bad])) and np.all(tri[~bad] >= 0)
    whole = bvh.nearest(T(dev, queries('soup65')))
    one = bvh.nearest(T(dev, queries('soup65')[7:8]))
    assert tuple(one.d2.shape) == (1,) and float(one.d2[0]) == float(whole.d2[7]) and int(one.tri[0]) == int(whole.tri[7])
    none = bvh.nearest(torch.zeros(0, 3, device=dev))
    assert tuple(none.d2.shape) == (0,) and tuple(none.bary.shape) == (0, 3)
    assert tuple(bvh.winding(torch.zeros(0, 3, device=dev)).shape) == (0,) and tuple(bvh.signed_distance(torch.zeros(0, 3, device=dev)).shape) == (0,)
    grid = bvh.nearest(T(dev, queries('soup65')).reshape(4, 250, 3).double())                 # leading dimensions, another float dtype
    assert tuple(grid.d2.shape) == (4, 250) and tuple(grid.bary.shape) == (4, 250, 3) and torch.equal(grid.tri.reshape(-1), whole.tri)
    assert tuple(bvh.winding(T(dev, queries('soup65')).reshape(4, 250, 3)).shape) == (4, 250)
    assert float(bvh.winding(T(dev, queries('soup65')[7:8]))[0]) == float(bvh.winding(T(dev, queries('soup65')))[7])


# ---- the read-back tree -----------------------------------------------------------------------------------------------------------------------------
class Tree:
    """nodes, tri9 and moments of a Bvh on the host; children from `nodes` alone (the right child is the rope of the left one)"""

    def __init__(self, bvh, moments=True):
        if moments:
            bvh.winding(torch.zeros(1, 3, device=bvh.device))                    # the moments are built at the first winding call
        self.F = F = bvh.F
        n = bvh.nodes.cpu().numpy().reshape(2 * F - 1, 2, 4)
        self.lo, self.hi = n[:, 0, :3], n[:, 1, :3]
        self.link, self.rope = n[:, 0, 3].copy().view(np.int32), n[:, 1, 3].copy().view(np.int32)
        self.tri9 = bvh.tri9.cpu().numpy().reshape(F, 3, 3)
        if moments:
            m = bvh.moments.cpu().numpy().reshape(2 * F - 1, 2, 4)
            self.c, self.r, self.n, self.area = m[:, 0, :3], m[:, 0, 3], m[:, 1, :3], m[:, 1, 3]
        self.left = np.where(self.link >= 0, self.link, -1)
        self.right = np.where(self.link >= 0, self.rope[np.maximum(self.link, 0)], -1)

    def leaves_below(self):
        """[2F-1] lists of leaf rows, by a post-order pass"""
        out = [None] * (2 * self.F - 1)
        stack = [0]
        while stack:
            k = stack[-1]
            if self.link[k] < 0:
                out[k] = [~int(self.link[k])]
                stack.pop()
            elif out[self.left[k]] is None or out[self.right[k]] is None:
                stack += [int(self.right[k]), int(self.left[k])]
            else:
                out[k] = out[self.left[k]] + out[self.right[k]]
                stack.pop()
        return out


def check_tree_and_leaf_map(dev, name):
    """leaf_tri maps the rows of tri9 back to the input; every node is reached once from the root"""
    v, f = mesh(name)
    bvh = build(dev, name)
    t = Tree(bvh, moments=False)
    leaf_tri = bvh.leaf_tri.cpu().numpy()
    assert leaf_tri.dtype == np.int32 and np.array_equal(np.sort(leaf_tri), np.arange(len(f)))
    want = v[f[leaf_tri].astype(np.int64)]
    rows = ~np.isnan(t.tri9).any((1, 2))
    assert np.array_equal(t.tri9[rows], want[rows])
    below = t.leaves_below()
    assert sorted(below[0]) == list(range(len(f)))


def check_moments(dev, name):
    v, f = mesh(name)
    bvh = build(dev, name)
    t = Tree(bvh)
    below = t.leaves_below()
    res = {}
    for dt in (np.float64, np.float32):
        tri = t.tri9.astype(dt)
        nv = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]) * dt(0.5)
        ar = np.sqrt((nv * nv).sum(1))
        dead = ~(ar > 0)
        nv[dead], ar[dead] = 0, 0
        cen = np.where(dead[:, None], 0, tri.sum(1) / dt(3))
        N, A, C = np.zeros((2 * t.F - 1, 3), dt), np.zeros(2 * t.F - 1, dt), np.zeros((2 * t.F - 1, 3), dt)
        for k, rows in enumerate(below):
            N[k], A[k] = nv[rows].sum(0, dtype=dt), ar[rows].sum(dtype=dt)
            if A[k] > 0:
                C[k] = (cen[rows] * ar[rows, None]).sum(0, dtype=dt) / A[k]
            elif t.lo[k, 0] <= t.hi[k, 0]:
                C[k] = (t.lo[k].astype(dt) + t.hi[k].astype(dt)) * dt(0.5)
        res[dt] = (N, A, C)
    (N, A, C), (N32, A32, C32) = res[np.float64], res[np.float32]
    assert_close(f'{name}: node area vectors n', t.n, N, N32)
    assert_close(f'{name}: node areas', t.area, A, A32)
    assert_close(f'{name}: node centres c', t.c, C, C32)
    worst = 0.0
    for k, rows in enumerate(below):
        p = t.tri9[rows].astype(np.float64).reshape(-1, 3)
        p = p[~np.isnan(p).any(1)]
        if len(p):
            far = np.linalg.norm(p - t.c[k].astype(np.float64), axis=1).max()
            worst = max(worst, far / t.r[k] if t.r[k] > 0 else np.inf)
            assert t.r[k] >= (1 - FLOOR) * far, (k, t.r[k], far)
        else:
            assert t.r[k] == 0 and np.all(t.c[k] == 0) and t.area[k] == 0
    print(f'{name}: max (distance from c to the farthest vertex below) / r over {2 * t.F - 1} nodes: {worst:.7f}')


# ---- winding number ---------------------------------------------------------------------------------------------------------------------------------
def walk(t, q, beta, dt):
    """the kernel's algorithm on the host, in dt, vectorised over the queries: -> (w in turns [N] float64, borderline [N] bool, nodes visited [N])"""
    q = q.astype(dt)
    N = len(q)
    acc, edge, visits = np.zeros(N, dt), np.zeros(N, bool), np.zeros(N, np.int64)
    c, r, nn, tri = t.c.astype(dt), t.r.astype(dt), t.n.astype(dt), t.tri9.astype(dt)
    stack = [(0, np.arange(N))]
    while stack:
        k, idx = stack.pop()
        if len(idx) == 0:
            continue
        visits[idx] += 1
        if t.link[k] < 0:
            row = tri[~int(t.link[k])]
            if not np.isnan(row).any():
                acc[idx] += solid_angles(q[idx], row[0][None], row[1][None], row[2][None])
            continue
        d = c[k][None] - q[idx]
        d2 = HC._dot(d, d)
        with np.errstate(over='ignore', invalid='ignore'):
            lim = (dt(beta) * r[k]) * (dt(beta) * r[k])
            far = d2 > lim
            if np.isfinite(lim):
                edge[idx] |= np.abs(d2 - lim) <= 1e-5 * lim
        fi = idx[far]
        acc[fi] += HC._dot(nn[k][None], d[far]) / (d2[far] * np.sqrt(d2[far]))
        stack += [(int(t.right[k]), idx[~far]), (int(t.left[k]), idx[~far])]          # left first: the rope walk's order
    return (acc / dt(4 * np.pi)).astype(np.float64), edge, visits


def check_winding_walk(dev, name, beta, kernel=True):
    """the kernel against the algorithm: w against the float64 host walk of the read-back tree, borderline queries left out (at most 1 %).
    kernel=False: the walker's side alone -- the cap on the share left out, on the CPU"""
    ref = reference(name)
    q = ref['q']
    bvh = build(dev, name)
    t = Tree(bvh)
    w64, edge, visits = walk(t, q, beta, np.float64)
    w32, edge32, _ = walk(t, q, beta, np.float32)
    keep = ~(edge | edge32)
    err = np.abs(w64 - ref['w64']).max()
    print(f'{name}, beta {beta}: {int((~keep).sum())} of {N_Q} queries borderline; nodes visited mean {visits.mean():.1f} max {visits.max()} of {2 * t.F - 1}; '
          f'|walk64 - w64| max {err:.3e} mean {np.abs(w64 - ref["w64"]).mean():.3e}')
    assert (~keep).mean() <= 0.01
    if not kernel:
        return err
    w = bvh.winding(T(dev, q), beta=beta)
    assert w.dtype == torch.float32 and tuple(w.shape) == (N_Q,)
    assert_close(f'{name}, beta {beta}: w against the float64 walk', w.cpu().numpy()[keep], w64[keep], w32[keep])
    return err


def check_winding_exact(dev, name):
    """beta = inf is the exact sum: against the float64 sum over all triangles; 1 inside and 0 outside the closed icosphere"""
    ref = reference(name)
    w = build(dev, name).winding(T(dev, ref['q']), beta=math.inf).cpu().numpy()
    if len(ref['live']) == 0:
        assert np.all(w == 0)
        return
    if np.abs(ref['w64']).max() == 0:
        assert np.all(w == 0)
        return
    assert_close(f'{name}: w at beta = inf against the float64 sum', w, ref['w64'], ref['w32'])
    if name == 'ico':
        rad = np.linalg.norm(ref['q'].astype(np.float64) - ICO_C, axis=1)
        inside = rad < 0.9 * ICO_R                                       # safely inside the faceted sphere
        outside = rad > ICO_R * 1.001
        assert inside.sum() > 50 and outside.sum() > 300
        assert_close('ico: w = 1 inside, 0 outside', w[inside | outside], inside[inside | outside].astype(np.float64), ref['w32'][inside | outside])


def sign_case(dev, name, beta=3.0):
    """-> (bvh, q, clear mask, wanted inside, tau) with tau = 2 max |walk64 - w64| from the float64 walker; the share left out is capped at 5 %"""
    ref = reference(name)
    bvh = build(dev, name)
    w64, _, _ = walk(Tree(bvh), ref['q'], beta, np.float64)
    tau = 2.0 * np.abs(w64 - ref['w64']).max()
    clear = np.abs(np.abs(ref['w64']) - 0.5) > tau
    print(f'{name}, beta {beta}: tau = {tau:.3e}; {int((~clear).sum())} of {N_Q} queries within tau of |w| = 0.5')
    assert (~clear).mean() <= 0.05
    return bvh, ref['q'], clear, np.abs(ref['w64']) > 0.5, tau


def check_sign(dev, name):
    bvh, q, clear, inside, _ = sign_case(dev, name)
    sdf = bvh.signed_distance(T(dev, q)).cpu().numpy()
    ref = reference(name)
    assert_close(f'{name}: |signed_distance| against the float64 loop', np.abs(sdf), ref['d64'], ref['d32'])
    bad = clear & (np.signbit(sdf) != inside)
    print(f'{name}: {int(inside.sum())} of {N_Q} queries inside; sign differs at {int(bad.sum())}')
    assert 50 < inside.sum() < N_Q - 50
    assert not bad.any(), np.nonzero(bad)[0][:10]


# ---- wiring -------------------------------------------------------------------------------------------------------------------------------------------
def check_mesh_wsdf_accel(dev, name):
    """mesh_wsdf(accel='bvh', beta=inf): mesh_wsdf's magnitude, and its sign outside the 1e-3 rad band; a passed Bvh is used, not rebuilt"""
    v, f = mesh(name)
    ref = reference(name)
    q, tv, tf = T(dev, ref['q']), T(dev, v), T(dev, f.astype(np.int32))
    sdf0, w0 = MO.mesh_wsdf(q, tv, tf)
    before = RT.BUILDS
    sdf1, w1 = MO.mesh_wsdf(q, tv, tf, accel='bvh', beta=math.inf)
    assert RT.BUILDS == before + 1
    bvh = RT.Bvh(tv, tf)
    before = RT.BUILDS
    sdf2, w2 = MO.mesh_wsdf(q, tv, tf, accel='bvh', beta=math.inf, bvh=bvh)
    assert RT.BUILDS == before and torch.equal(sdf1, sdf2) and torch.equal(w1, w2)
    only_w = MO.mesh_wsdf(q, tv, tf, want_sdf=False, accel='bvh', bvh=bvh)
    assert only_w[0] is None and tuple(only_w[1].shape) == (N_Q,)
    sdf0, w0, sdf1, w1 = (x.cpu().numpy() for x in (sdf0, w0, sdf1, w1))
    assert_close(f'{name}: |sdf| of accel = bvh against the float64 loop', np.abs(sdf1), ref['d64'], ref['d32'])
    print(f'{name}: {int((np.abs(sdf0).view(np.uint32) != np.abs(sdf1).view(np.uint32)).sum())} magnitudes differ in their bits from accel = brute')
    assert_close(f'{name}: w of accel = bvh, beta = inf against the float64 sum', w1, ref['w64'], ref['w32'])
    clear = np.abs(np.abs(w0.astype(np.float64)) - 0.5) * 4 * np.pi > 1e-3
    bad = clear & (np.signbit(sdf0) != np.signbit(sdf1))
    print(f'{name}: {int((~clear).sum())} queries within 1e-3 rad of the decision; sign differs from accel = brute at {int(bad.sum())}')
    assert not bad.any()


def check_defaults_are_untouched(dev):
    """with every accel left at its default no BVH is built and mesh_wsdf's bits are those of the entry point called directly"""
    v, f = mesh('ico_open')
    q, tv, tf = T(dev, queries('ico_open')), T(dev, v), T(dev, f.astype(np.int32))
    before = RT.BUILDS
    sdf, w = MO.mesh_wsdf(q, tv, tf)
    raw_s, raw_w = torch.empty_like(sdf), torch.empty_like(w)
    L.call('mesh_wsdf', q, N_Q, tv, tf, len(f), raw_s, raw_w)
    assert torch.equal(sdf.view(torch.int32), raw_s.view(torch.int32)) and torch.equal(w.view(torch.int32), raw_w.view(torch.int32))
    from d3h import tetfill as TF, watertight as WT
    WT.extract(tv, tf, res=8)
    TF.fill_mesh(tv, tf, res=8)
    import script.process_body_cloth_head_msdfcut as PB
    PB.GarmentField(v, f).device(q[:8])
    assert RT.BUILDS == before


def check_watertight_accel(dev):
    """watertight(accel='bvh') on the capsule pieces at the smallest res the scenario is tested at: closed, outward-wound, Euler characteristic 2, every
    non-cap vertex within h / 4 of the input"""
    from d3h import meshtopo as MT, watertight as WT
    res = 32
    v, f, h = HC.capsule_pieces(res)
    v = v.astype(np.float32)
    before = RT.BUILDS
    wv, wf, cap = WT.watertight(T(dev, v), T(dev, f), res=res, relax_iters=32, accel='bvh')
    assert RT.BUILDS == before + 1                                         # one tree for both queries
    assert len(MT.open_vertices(wf, len(wv))) == 0
    wv, wf, cap = wv.cpu().numpy(), wf.cpu().numpy(), cap.cpu().numpy()
    e, c = HC._edges(wf)
    assert np.all(c == 2)
    assert HC._signed_volume(wv, wf) > 0
    chi = len(np.unique(wf)) - len(e) + len(wf)
    d = HC.dist_upper_bound(wv[~cap], v, f)
    print(f'watertight(accel = bvh): {len(wv)} vertices, {int(cap.sum())} cap vertices, Euler characteristic {chi}, non-cap distance at most {d.max() / h:.3f} h')
    assert chi == 2 and len(np.unique(wf)) == len(wv)
    assert cap.any() and d.max() <= h / 4 + FLOOR


def check_garment_field_builds_once(dev):
    """three push rounds on a GarmentField(accel='bvh'): one build; the pushed vertices are those of the brute field away from the |w| = 0.5 band"""
    import script.process_body_cloth_head_msdfcut as PB
    v, f = mesh('ico_open')
    rng = OC._rng('bvhdist push')
    d = rng.standard_normal((300, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[:, 2] = -np.abs(d[:, 2])                                             # below the opening
    pts = (ICO_C + ICO_R * rng.uniform(0.97, 1.03, (300, 1)) * d).astype(np.float32)
    nrm = d.astype(np.float32)
    before = RT.BUILDS
    field = PB.GarmentField(v, f, accel='bvh')
    out, pushes = MO.collision_push(T(dev, pts), T(dev, nrm), field.device, eps=0.005, margin=0.002, rounds=3, stop_when_still=False)
    assert RT.BUILDS == before + 1
    out0, pushes0 = MO.collision_push(T(dev, pts), T(dev, nrm), PB.GarmentField(v, f).device, eps=0.005, margin=0.002, rounds=3, stop_when_still=False)
    assert RT.BUILDS == before + 1
    same = torch.equal(pushes, pushes0)
    print(f'garment field, 3 rounds: {int(pushes.sum())} pushes with accel = bvh, {int(pushes0.sum())} with brute; identical: {same}')
    assert int(pushes.sum()) > 100 and same and torch.equal(out, out0)
    with pytest.raises(RuntimeError):
        PB.GarmentField(v, f, accel='octree')


def check_validation(dev, monkeypatch):
    """bad shapes, beta <= 0 or NaN, points or a Bvh on another device: RuntimeError before any native call"""
    bvh = build(dev, 'soup3')
    v, f = mesh('soup3')
    q = torch.zeros(4, 3, device=dev)
    bvh.winding(q)                                                         # the moments exist: nothing below may reach the library
    monkeypatch.setattr(L, 'call', lambda *a: pytest.fail(f'native call {a[0]}'))
    for fn in (bvh.nearest, bvh.winding, bvh.signed_distance):
        for bad in (torch.zeros(4, 2, device=dev), torch.tensor(0.0, device=dev), torch.zeros(4, 3, dtype=torch.int32, device=dev),
                    torch.zeros(4, 3, device='meta'), [[0.0, 0.0, 0.0]]):
            with pytest.raises(RuntimeError):
                fn(bad)
    for fn in (bvh.winding, bvh.signed_distance):
        for beta in (0.0, -1.0, float('nan')):
            with pytest.raises(RuntimeError):
                fn(q, beta=beta)
    tv, tf = T(dev, v), T(dev, f)
    with pytest.raises(RuntimeError):
        MO.mesh_wsdf(q, tv, tf, accel='kd')
    with pytest.raises(RuntimeError):
        MO.mesh_wsdf(q, tv, tf, accel='bvh', beta=0.0, bvh=bvh)
    with pytest.raises(RuntimeError):
        MO.mesh_wsdf(q, tv, tf, accel='bvh', bvh='not a Bvh')
    with pytest.raises(RuntimeError):
        MO.mesh_wsdf(q, tv, tf[:2], accel='bvh', bvh=bvh)                  # a tree of another mesh
    with pytest.raises(RuntimeError):
        MO.mesh_wsdf(torch.zeros(4, 3, device='meta'), tv, tf, accel='bvh', bvh=bvh)


def check_flag_mesh_sdf_accel(dev):
    """FLAGS.mesh_sdf_accel = 'bvh' reaches both queries of _init_tet_smpl (the lattice field of fill_mesh, sdf_tet_gt); absent, no BVH is built.  The
    template is closed and has no zero-area triangle, so the distances are the brute-force bits and no lattice vertex is near |w| = 0.5: same tet mesh"""
    import os
    import tetfill_startup_cases as TS
    from conftest import GOLD
    from d3h.scene import Scene

    def make(accel):
        def hook(F):
            F.prefit_with_library_path, F.eikonal_samples = True, 96
            F.smplx_model_dict = TS.body_model(True)
            F.out_dir = None
            F.tet_smpl, F.tet_smpl_res = True, 8
            if accel is not None:
                F.mesh_sdf_accel = accel
        torch.manual_seed(0)
        before = RT.BUILDS
        sc = Scene(res=32, grid_n=6, n_frames=1, device=dev, seed=0, prefit_steps=0, loss_set='mask', body_verts=258, sdf_fn=TS.ELL, flags_hook=hook,
                   sdf_state=os.path.join(GOLD, 'parity_state_sdf.npz'))
        return sc.geometry, RT.BUILDS - before
    g0, b0 = make(None)
    g1, b1 = make('bvh')
    print(f'FLAGS.mesh_sdf_accel absent: {b0} BVH builds; bvh: {b1}; {g1.tet_smpl_v.shape[0]} tet vertices')
    assert b0 == 0 and b1 == 2
    assert torch.equal(g0.tet_smpl_v, g1.tet_smpl_v) and torch.equal(g0.tet_smpl_f, g1.tet_smpl_f)
    assert torch.equal(g0.sdf_tet_gt, g1.sdf_tet_gt)
