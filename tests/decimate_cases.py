"""Check functions of quadric decimation (csrc/meshdecim.hip, d3h.meshrefine.decimate) and of the level-of-detail export chain (d3h.export.lod_chain),
shared by tests/test_decimate_emul.py (host emulation of the kernel sources) and tests/test_gpu_decimate.py (MI355X).  Same shapes on both.  Every mesh
is generated here or in remesh_cases.py from a seed.

Yardsticks:
  decimate     a sequential numpy restatement of the docstring of d3h.meshrefine: float64 in the stated order (numpy rounds every elementwise
               operation once), an explicit Cramer's rule, no np.linalg.  Selection is a minimum over sets and the trim a prefix of a sorted list, so
               the restatement has no notion of parallelism.  EXACT: faces, parent and vmap as integers, positions bit for bit, info equal; the
               quadrics per vertex bit for bit.
  quality      the classic algorithm: the cheapest candidate of the WHOLE mesh (same quadrics, placement, classes and checks, every cost re-evaluated
               after every collapse, ties to the smaller rank) collapses, one at a time.  Distances are float64 brute-force closest points
               (remesh_cases.closest_points) from the vertices and face centroids of one mesh to the other, as RMS.
The emulator runs the threads of a launch one after another, so it cannot show a race: the contended cases count on the GPU."""
import functools
import math

import numpy as np
import pytest
import torch

import handoff_cases as HC
import remesh_cases as RC
from d3h import meshrefine as MR

F32, F64 = np.float32, np.float64
FREE = np.uint64(0x7fffffffffffffff)
U32 = np.uint64(0xffffffff)


# ---- meshes -----------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cube(k):
    """the cube [-1, 1]^3 with k x k quads per side, 12 k^2 faces, outward; every coordinate is a multiple of 2 / k and exact in float32 for k = 4, 8"""
    idx, v, f = {}, [], []

    def vid(p):
        if p not in idx:
            idx[p] = len(v)
            v.append(p)
        return idx[p]
    for axis in range(3):
        for side in (-1, 1):
            for i in range(k):
                for j in range(k):
                    def pt(a, b):
                        p = [0, 0, 0]
                        p[axis], p[(axis + 1) % 3], p[(axis + 2) % 3] = side * k, 2 * a - k, 2 * b - k
                        return vid(tuple(p))
                    q = [pt(i, j), pt(i + 1, j), pt(i + 1, j + 1), pt(i, j + 1)]
                    if side < 0:
                        q = q[::-1]
                    f += [(q[0], q[1], q[2]), (q[0], q[2], q[3])]
    v, f = np.array(v, F64) / k, np.array(f, np.int64)
    assert HC._signed_volume(v, f) > 0 and len(f) == 12 * k * k
    return v.astype(F32), f


@functools.lru_cache(maxsize=None)
def lumpy_sphere():
    """icosphere(3), 1280 faces, scaled by 1 + 0.25 sin(3 theta) sin(2 phi), then by (1, 0.7, 1.4)"""
    v, f = RC._icosphere(3)
    theta, phi = np.arccos(np.clip(v[:, 2], -1, 1)), np.arctan2(v[:, 1], v[:, 0])
    p = v * (1 + 0.25 * np.sin(3 * theta) * np.sin(2 * phi))[:, None] * np.array([1.0, 0.7, 1.4])
    return p.astype(F32), f


@functools.lru_cache(maxsize=None)
def ico(level):
    v, f = RC._icosphere(level)
    return v.astype(F32), f


# ---- the restatement --------------------------------------------------------------------------------------------------------------------------
def det3(m00, m01, m02, m10, m11, m12, m20, m21, m22):
    return (m00 * (m11 * m22 - m12 * m21) - m01 * (m10 * m22 - m12 * m20)) + m02 * (m10 * m21 - m11 * m20)


def error(Q, q):
    x, y, z = q[..., 0], q[..., 1], q[..., 2]
    rx = (Q[..., 0] * x + Q[..., 1] * y) + Q[..., 2] * z
    ry = (Q[..., 1] * x + Q[..., 4] * y) + Q[..., 5] * z
    rz = (Q[..., 2] * x + Q[..., 5] * y) + Q[..., 7] * z
    e = (((x * rx + y * ry) + z * rz) + 2.0 * ((Q[..., 3] * x + Q[..., 6] * y) + Q[..., 8] * z)) + Q[..., 9]
    return np.where(e < 0, 0.0, e)


def _plane(u, d, w):
    return np.stack([w * (u[:, 0] * u[:, 0]), w * (u[:, 0] * u[:, 1]), w * (u[:, 0] * u[:, 2]), w * (u[:, 0] * d), w * (u[:, 1] * u[:, 1]), w * (u[:, 1] * u[:, 2]),
                     w * (u[:, 1] * d), w * (u[:, 2] * u[:, 2]), w * (u[:, 2] * d), w * (d * d)], 1)


class Topology:
    """the adjacency of the docstring as numpy arrays: sorted unique edges with counts, the two CSR rows, the classes"""

    def __init__(self, f, n, pin, slide):
        f = np.asarray(f, np.int64).reshape(-1, 3)
        a, b = f.reshape(-1), f[:, [1, 2, 0]].reshape(-1)
        self.side_keys = (np.minimum(a, b) << 32) | np.maximum(a, b)
        self.keys, self.cnt = np.unique(self.side_keys, return_counts=True)
        self.elo, self.ehi = self.keys >> 32, self.keys & 0xffffffff
        proper = self.elo != self.ehi
        nk = np.sort(np.concatenate([self.keys[proper], (self.ehi[proper] << 32) | self.elo[proper]]))
        self.nbr = nk & 0xffffffff
        self.val = np.bincount(nk >> 32, minlength=n)
        self.noffs = np.concatenate([[0], np.cumsum(self.val)])
        fk = np.unique((a << 32) | np.repeat(np.arange(len(f)), 3))
        self.vf = fk & 0xffffffff
        self.fdeg = np.bincount(fk >> 32, minlength=n)
        self.foffs = np.concatenate([[0], np.cumsum(self.fdeg)])
        pinned = np.zeros(n, bool) if pin is None else np.asarray(pin, bool).copy()
        fixed = (self.cnt > 2) | ~proper
        pinned[self.elo[fixed]] = True
        pinned[self.ehi[fixed]] = True
        op = (self.cnt == 1) & proper
        nopen = np.bincount(np.concatenate([self.elo[op], self.ehi[op]]), minlength=n)
        pinned |= ((nopen != 0) & (nopen != 2)) if slide else (nopen != 0)
        self.vclass = np.where(pinned, 2, np.where(nopen == 2, 1, 0))

    def has_edge(self, x, y):
        k = (np.minimum(x, y) << 32) | np.maximum(x, y)
        at = np.minimum(np.searchsorted(self.keys, k), len(self.keys) - 1)
        return self.keys[at] == k


def _rows(offs, deg, items, owners):
    """the CSR rows of `owners`, flattened: (which owner each entry belongs to, the entries)"""
    cnt = deg[owners]
    rep = np.repeat(np.arange(len(owners)), cnt)
    pos = np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    return rep, items[offs[owners][rep] + pos]


def quadrics_yardstick(v, f, slide):
    v, f = np.asarray(v, F32), np.asarray(f, np.int64).reshape(-1, 3)
    n, p = len(v), np.asarray(v, F32).astype(F64)
    T = Topology(f, n, None, slide)
    Q = np.zeros((n, 10), F64)
    with np.errstate(all='ignore'):
        p0 = p[f[:, 0]]
        nr = RC._cross(p[f[:, 1]] - p0, p[f[:, 2]] - p0)
        l = np.sqrt(RC._dot(nr, nr))
        ok = l > 0
        u = nr / l[:, None]
        K = _plane(u, -RC._dot(u, p0), l * 0.5)
        vert = np.repeat(np.arange(n), T.fdeg)
        pos = np.arange(len(T.vf)) - T.foffs[vert]
        for k in range(int(T.fdeg.max()) if n else 0):                             # the k-th face of every vertex: ascending face index, from 0
            m = (pos == k) & ok[T.vf]
            Q[vert[m]] = Q[vert[m]] + K[T.vf[m]]
        if slide:
            op = np.nonzero((T.cnt == 1) & (T.elo != T.ehi))[0]
            a, b = T.elo[op], T.ehi[op]
            order = np.argsort(T.side_keys, kind='stable')
            face = (order[np.searchsorted(T.side_keys[order], T.keys[op])]) // 3   # the one face of each open edge
            e = p[b] - p[a]
            m = RC._cross(e, u[face])
            lm = np.sqrt(RC._dot(m, m))
            good = ok[face] & (lm > 0)
            mu = m / lm[:, None]
            B = _plane(mu, -RC._dot(mu, p[a]), 4.0 * RC._dot(e, e))
            ends = np.concatenate([a, b])
            which = np.concatenate([np.arange(len(op)), np.arange(len(op))])
            o = np.lexsort((which, ends))                                          # per vertex, ascending rank (op is ascending)
            ends, which = ends[o], which[o]
            first = np.searchsorted(ends, ends)
            posb = np.arange(len(ends)) - first
            for k in range(int(posb.max()) + 1 if len(ends) else 0):
                m_ = (posb == k) & good[which]
                Q[ends[m_]] = Q[ends[m_]] + B[which[m_]]
    return Q


def mix(rank, rnd):
    x = (rank.astype(np.uint64) ^ np.uint64((rnd * 0x9e3779b9) & 0xffffffff)) & U32
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x85ebca6b)) & U32
    x ^= x >> np.uint64(13)
    x = (x * np.uint64(0xc2b2ae35)) & U32
    x ^= x >> np.uint64(16)
    return x


def evaluate(v, f, Q, pin, slide, max_cost):
    """every edge's class, placement, cost and checks -> (Topology, candidate mask, cost float64, q float32, survivor, Qe)"""
    n = len(v)
    T = Topology(f, n, pin, slide)
    a, b, cnt = T.elo, T.ehi, T.cnt
    ca, cb = T.vclass[a], T.vclass[b]
    proper = a != b
    k1 = proper & (cnt == 2) & (ca == 0) & (cb == 0)
    k2 = proper & (cnt == 2) & ((ca == 0) != (cb == 0))
    k3 = proper & (cnt == 1) & bool(slide) & (ca == 1) & (cb == 1)
    Qe = Q[a] + Q[b]
    A32, B32 = v[a], v[b]
    Ad, Bd = A32.astype(F64), B32.astype(F64)
    with np.errstate(all='ignore'):
        m = [Qe[:, i] for i in range(10)]
        det = det3(m[0], m[1], m[2], m[1], m[4], m[5], m[2], m[5], m[7])
        t = (m[0] + m[4]) + m[7]
        mid = (Ad + Bd) * 0.5
        r0, r1, r2 = -m[3], -m[6], -m[8]
        x = np.stack([det3(r0, m[1], m[2], r1, m[4], m[5], r2, m[5], m[7]) / det, det3(m[0], r0, m[2], m[1], r1, m[5], m[2], r2, m[7]) / det,
                      det3(m[0], m[1], r0, m[1], m[4], r1, m[2], m[5], r2) / det], 1)
        take = (np.abs(det) > 1e-9 * ((t * t) * t)) & np.isfinite(x).all(1) & (RC._len2(x, mid) <= 4.0 * RC._len2(Ad, Bd))
        cost = np.full(len(a), np.inf)
        q = np.zeros((len(a), 3), F32)
        for opt, allowed in ((x.astype(F32), take), (mid.astype(F32), True), (A32, True), (B32, True)):
            e = error(Qe, opt.astype(F64))
            better = allowed & (e < cost)
            cost, q = np.where(better, e, cost), np.where(better[:, None], opt, q)
        surv = a.copy()
        fixed_a = ca != 0
        q2 = np.where(fixed_a[:, None], A32, B32)
        cost = np.where(k2, error(Qe, q2.astype(F64)), cost)
        q, surv = np.where(k2[:, None], q2, q), np.where(k2 & ~fixed_a, b, surv)
        ea, eb = error(Qe, Ad), error(Qe, Bd)
        pick_b = eb < ea
        cost = np.where(k3, np.where(pick_b, eb, ea), cost)
        q, surv = np.where(k3[:, None], np.where(pick_b[:, None], B32, A32), q), np.where(k3 & pick_b, b, surv)
        ok = (k1 | k2 | k3) & np.isfinite(cost) & (cost <= max_cost)
    R = np.nonzero(ok)[0]
    if len(R):                                                                     # link
        want = np.where(cnt[R] == 1, 1, 2)
        rep, x_ = _rows(T.noffs, T.val, T.nbr, a[R])
        shared = T.has_edge(x_, b[R][rep]) & (x_ != b[R][rep])
        common = np.bincount(rep, shared, minlength=len(R))
        thin = np.bincount(rep, shared & (T.val[x_] <= want[rep] + 1), minlength=len(R))
        ok[R[(common != want) | (thin > 0)]] = False
    R = np.nonzero(ok)[0]
    for end, other in ((a, b), (b, a)):                                            # normal, float32
        if not len(R):
            break
        rep, faces = _rows(T.foffs, T.fdeg, T.vf, end[R])
        rows = f[faces]
        skip = (rows == other[R][rep][:, None]).any(1)
        P = v[rows]
        Pn = np.where((rows == end[R][rep][:, None])[..., None], q[R][rep][:, None, :], P)
        good = skip | RC._cos_ok(RC._nrm(P[:, 0], P[:, 1], P[:, 2]), RC._nrm(Pn[:, 0], Pn[:, 1], Pn[:, 2]), F32(0.04))
        assert P.dtype == np.float32 and Pn.dtype == np.float32
        ok[R[np.bincount(rep, ~good, minlength=len(R)) > 0]] = False
    return T, ok, cost, q, surv, Qe


def _collapse(T, f, r, surv, q, Qe, vout, Qout, remap, drop):
    a, b = int(T.elo[r]), int(T.ehi[r])
    s = int(surv[r])
    o = b if s == a else a
    vout[s], Qout[s], remap[o] = q[r], Qe[r], s
    fa = T.vf[T.foffs[a]:T.foffs[a + 1]]
    drop[fa[(f[fa] == b).any(1)]] = True


def _compact(vout, Qout, f, remap, drop):
    n = len(vout)
    keep = remap == np.arange(n)
    newidx = np.cumsum(keep) - 1
    return vout[keep], newidx[remap[f[~drop]]], np.nonzero(~drop)[0], newidx[remap], keep, Qout[keep]


def decimate_round_yardstick(v, f, Q, pin, target, window, min_window, slide, max_cost, rnd, stats=None):
    n, nf = len(v), len(f)
    T, cand, cost, q, surv, Qe = evaluate(v, f, Q, pin, slide, max_cost)
    ne = len(T.keys)
    rank = np.arange(ne, dtype=np.uint64)
    bits = cost.astype(F32).view(np.uint32).astype(np.uint64)
    wkey = np.where(cand, (bits << np.uint64(32)) | rank, FREE)
    need = (nf - target + 1) // 2
    w = min(max(int(math.ceil(window * need)), min_window), ne)
    thr = np.sort(wkey)[w - 1]
    inside = np.nonzero(cand & (wkey <= thr))[0].tolist()
    ekey = ((bits >> np.uint64(20)) << np.uint64(32)) | mix(rank, rnd)
    sets = [{int(T.elo[r]), int(T.ehi[r])} | set(T.nbr[T.noffs[T.elo[r]]:T.noffs[T.elo[r] + 1]].tolist()) | set(T.nbr[T.noffs[T.ehi[r]]:T.noffs[T.ehi[r] + 1]].tolist())
            for r in inside]
    selected = sorted(RC._select(n, inside, ekey, sets), key=lambda r: int(ekey[r]))
    vout, Qout, remap, drop = v.copy(), Q.copy(), np.arange(n), np.zeros(nf, bool)
    done, gone, worst = 0, 0, 0.0
    for r in selected:                                                             # the trim: a prefix
        if gone + int(T.cnt[r]) > nf - target:
            break
        _collapse(T, f, r, surv, q, Qe, vout, Qout, remap, drop)
        done, gone, worst = done + 1, gone + int(T.cnt[r]), max(worst, float(cost[r]))
    if stats is not None:
        stats.append((int(cand.sum()), len(inside), len(selected), done))
    if done == 0:
        return None
    assert gone == drop.sum()
    return _compact(vout, Qout, f, remap, drop) + (done, worst)


def decimate_yardstick(v, f, target, rounds=256, window=3.0, min_window=256, boundary='slide', max_cost=np.inf, pin=None, stats=None):
    v, f = np.asarray(v, F32), np.asarray(f, np.int64).reshape(-1, 3)
    slide = boundary == 'slide'
    parent, vmap = np.arange(len(f)), np.arange(len(v))
    pin = None if pin is None else np.asarray(pin, bool)
    info = dict(rounds=0, collapses=0, reached=True, max_cost=0.0)
    if len(f) <= target:
        return v, f, parent, vmap, info
    Q = quadrics_yardstick(v, f, slide)
    for rnd in range(rounds):
        if len(f) <= target:
            break
        r = decimate_round_yardstick(v, f, Q, pin, target, window, min_window, slide, max_cost, rnd, stats)
        if r is None:
            break
        v, f, p, m, keep, Q, nc, worst = r
        parent, vmap = parent[p], m[vmap]
        pin = None if pin is None else pin[keep]
        info['rounds'] += 1
        info['collapses'] += nc
        info['max_cost'] = max(info['max_cost'], worst)
    info['reached'] = len(f) <= target + 1
    return v, f, parent, vmap, info


def greedy_yardstick(v, f, targets, boundary='slide'):
    """the classic algorithm (module docstring) -> {target: (v, f)} for the descending face counts `targets`"""
    v, f = np.asarray(v, F32), np.asarray(f, np.int64).reshape(-1, 3)
    slide = boundary == 'slide'
    Q = quadrics_yardstick(v, f, slide)
    out = {}
    for target in sorted(targets, reverse=True):
        while len(f) > target:
            T, cand, cost, q, surv, Qe = evaluate(v, f, Q, None, slide, np.inf)
            cand &= T.cnt <= len(f) - target
            if not cand.any():
                break
            r = int(np.lexsort((np.arange(len(cost)), np.where(cand, cost, np.inf)))[0])
            vout, Qout, remap, drop = v.copy(), Q.copy(), np.arange(len(v)), np.zeros(len(f), bool)
            _collapse(T, f, r, surv, q, Qe, vout, Qout, remap, drop)
            v, f, _, _, _, Q = _compact(vout, Qout, f, remap, drop)
        out[target] = (v, f)
    return out


# ---- figures --------------------------------------------------------------------------------------------------------------------------------------
def _points(v, f):
    v = np.asarray(v, F64)
    return np.concatenate([v[np.unique(f)], v[f].mean(1)])


def rms_pair(v0, f0, v1, f1):
    """(RMS distance from mesh 1's vertices and centroids to mesh 0, from mesh 0's to mesh 1), float64 brute force"""
    out = []
    for (pv, pf), (sv, sf) in (((v1, f1), (v0, f0)), ((v0, f0), (v1, f1))):
        p = _points(pv, pf)
        c = RC.closest_points(p, np.asarray(sv, F64), np.asarray(sf, np.int64))[0]
        out.append(float(np.sqrt(((c - p) ** 2).sum(1).mean())))
    return tuple(out)


def volume(v, f):
    return HC._signed_volume(np.asarray(v, F64), np.asarray(f, np.int64))


def _loops(f):
    """the number of boundary loops: components of the graph of open edges"""
    e, c = HC._edges(np.asarray(f, np.int64))
    e = e[c == 1]
    root = {}

    def find(x):
        while root.setdefault(x, x) != x:
            root[x] = root[root[x]]
            x = root[x]
        return x
    for a, b in e.tolist():
        root[find(a)] = find(b)
    return len({find(x) for x in root})


def check_invariants(v0, f0, v1, f1, parent, vmap, target, pin=None, boundary='slide', closed=False):
    """issue item 4, from the returned arrays alone"""
    v0, v1, f0, f1 = np.asarray(v0, F32), np.asarray(v1, F32), np.asarray(f0, np.int64), np.asarray(f1, np.int64)
    assert len(f1) >= min(target, len(f0)) and f1.min() >= 0 and f1.max() < len(v1)
    assert np.all((f1[:, 0] != f1[:, 1]) & (f1[:, 1] != f1[:, 2]) & (f1[:, 2] != f1[:, 0]))
    assert len(np.unique(np.sort(f1, 1), axis=0)) == len(f1)                                                          # no duplicate face
    c0, c1 = HC._edges(f0)[1], HC._edges(f1)[1]
    assert c1.max() <= max(2, c0.max()) and (c1 > 2).sum() == (c0 > 2).sum()
    assert HC._euler(f1) == HC._euler(f0) and _loops(f1) == _loops(f0)
    if closed:
        assert np.all(c1 == 2) and volume(v1, f1) * volume(v0, f0) > 0
    b0 = {tuple(x) for x in RC._bits(v0[np.unique(HC._edges(f0)[0][c0 == 1])]).tolist()}
    b1 = {tuple(x) for x in RC._bits(v1[np.unique(HC._edges(f1)[0][c1 == 1])]).tolist()}
    assert b1 <= b0                                                                                                   # boundary vertices thin out, none moves
    assert len(parent) == len(f1) and np.all(np.diff(parent) > 0) and parent.min() >= 0 and parent.max() < len(f0)
    assert len(vmap) == len(v0) and vmap.min() >= 0 and vmap.max() < len(v1)
    assert np.array_equal(vmap[f0[parent]], f1)                                                                       # a kept face is its parent, renumbered
    pinned = Topology(f0, len(v0), pin, boundary == 'slide').vclass == 2
    assert np.array_equal(RC._bits(v1[vmap[pinned]]), RC._bits(v0[pinned]))
    first = np.full(len(v1), len(v0))
    np.minimum.at(first, vmap, np.arange(len(v0)))
    assert np.all(first < len(v0))                                                                                    # every output vertex was an input vertex


# ---- drivers of the code under test -----------------------------------------------------------------------------------------------------------
def run(dev, v, f, target, dtype=torch.int64, pin=None, **kw):
    tv, tf, tp = RC._t(dev, v, f, dtype, pin)
    gv, gf, gp, gm, info = MR.decimate(tv, tf, target, pin_mask=tp, **kw)
    assert gf.dtype == dtype and gp.dtype == torch.int64 and gm.dtype == torch.int64 and gv.dtype == torch.float32
    assert np.array_equal(tf.cpu().numpy(), np.asarray(f).reshape(-1, 3)) and np.array_equal(RC._bits(tv.cpu().numpy()), RC._bits(v))      # inputs not written
    return gv.cpu().numpy(), gf.cpu().numpy().astype(np.int64), gp.cpu().numpy(), gm.cpu().numpy(), info


def _equal(dev, v, f, target, dtype=torch.int64, pin=None, stats=None, closed=False, **kw):
    yv, yf, yp, ym, yi = decimate_yardstick(v, f, target, pin=pin, stats=stats, **kw)
    gv, gf, gp, gm, gi = run(dev, v, f, target, dtype, pin, **kw)
    assert gf.shape == yf.shape and np.array_equal(gf, yf)
    assert np.array_equal(gp, yp) and np.array_equal(gm, ym)
    assert gv.shape == yv.shape and np.array_equal(RC._bits(gv), RC._bits(yv))
    assert gi == yi, (gi, yi)
    if len(f):
        check_invariants(v, f, gv, gf, gp, gm, target, pin, kw.get('boundary', 'slide'), closed)
    again = run(dev, v, f, target, dtype, pin, **kw)
    assert all(np.array_equal(x, y) for x, y in zip(again[:4], (gv, gf, gp, gm))) and np.array_equal(RC._bits(again[0]), RC._bits(gv)) and again[4] == gi
    return gv, gf, gp, gm, gi


# ---- checks -------------------------------------------------------------------------------------------------------------------------------------
def check_quadrics(dev):
    """per vertex, bit for bit: closed, open under 'slide' (boundary planes) and 'pin', a zero-area face, int32 faces"""
    sv, sf = RC.sphere_case(True)
    flat = (np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [0, 1, 0]], F32), np.array([[0, 1, 2], [0, 1, 3]], np.int64))
    for (v, f), slide, dtype in ((ico(2), True, torch.int64), ((sv, sf), True, torch.int32), ((sv, sf), False, torch.int64), (flat, True, torch.int64),
                                 (cube(4), True, torch.int32)):
        tv, tf, _ = RC._t(dev, v, f, dtype)
        Q, counts = MR._quadrics(tv, tf, slide)
        y = quadrics_yardstick(v, f, slide)
        assert counts.tolist()[2] == 0 and np.array_equal(Q.cpu().numpy().view(np.uint64), y.view(np.uint64))
    open_v = np.unique(HC._edges(sf)[0][HC._edges(sf)[1] == 1])
    assert len(open_v) and not np.array_equal(quadrics_yardstick(sv, sf, True)[open_v], quadrics_yardstick(sv, sf, False)[open_v])


def check_icosphere(dev):
    stats = []
    v, f = ico(2)
    gv, gf, _, _, info = _equal(dev, v, f, 80, stats=stats, closed=True)
    print('icosphere(2) 320 -> 80: (candidates, in the window, selected, applied) per round', stats, info)
    assert len(gf) == 80 and info['reached']


def check_cube_ties(dev):
    """4 x 4 quads per side, every cost 0: the hashed rank and the trim decide"""
    stats = []
    v, f = cube(4)
    gv, gf, _, _, info = _equal(dev, v, f, 24, stats=stats, closed=True)
    print('cube(4) 192 -> 24:', stats, info)
    assert len(gf) == 24 and info['max_cost'] == 0.0 and stats[0][2] > 1                                               # a rank tie-break selects one per chain of ties


def check_open(dev, boundary):
    v, f = RC.sphere_case(True)
    stats = []
    target = 400
    gv, gf, gp, gm, info = _equal(dev, v, f, target, torch.int32, stats=stats, boundary=boundary)
    n_open = lambda ff: int((HC._edges(ff)[1] == 1).sum())
    print(f'open sphere {len(f)} -> {len(gf)} ({boundary}): {info}, open edges {n_open(f)} -> {n_open(gf)}')
    assert info['reached'] and (n_open(gf) < n_open(f) if boundary == 'slide' else n_open(gf) == n_open(f))


def check_sheet(dev, k):
    """a min_window of k lets exactly k candidates claim: 64 / 65 a wave's edge, 300 a workgroup's"""
    v, f = RC._sheet(300)
    stats = []
    _equal(dev, v, f, len(f) // 2, torch.int32 if k == 65 else torch.int64, stats=stats, rounds=2, window=1e-9, min_window=k)
    print(f'sheet, window {k}:', stats)
    assert stats[0][1] == k and 0 < stats[0][2] < k


def check_pin_mask(dev):
    v, f = ico(2)
    pin = np.random.default_rng(11).random(len(v)) < 0.2
    gv, gf, gp, gm, info = _equal(dev, v, f, 160, pin=pin, closed=True)
    free = _equal(dev, v, f, 160, closed=True)
    assert not np.array_equal(gf, free[1]) and info['reached']


def check_trim(dev):
    """a target two faces below the input, then one a single round overshoots: the trim cuts inside the round"""
    v, f = ico(2)
    for target in (318, 310, 311):
        stats = []
        gv, gf, _, _, info = _equal(dev, v, f, target, stats=stats, closed=True)
        print(f'trim 320 -> {target}:', stats, info)
        assert stats[0][3] < stats[0][2] and len(gf) in (target, target + 1) and info['rounds'] == 1


def check_small(dev):
    """target >= F, F = 0, a single triangle, a tetrahedron: nothing may collapse"""
    v, f = ico(2)
    for target in (320, 1000):
        gv, gf, gp, gm, info = _equal(dev, v, f, target)
        assert np.array_equal(gf, f) and np.array_equal(RC._bits(gv), RC._bits(v)) and info == dict(rounds=0, collapses=0, reached=True, max_cost=0.0)
    gv, gf, gp, gm, info = _equal(dev, np.zeros((3, 3), F32), np.zeros((0, 3), np.int64), 0)
    assert gv.shape == (3, 3) and gf.shape == (0, 3) and gp.shape == (0,) and np.array_equal(gm, np.arange(3))
    tri = (np.array([[0, 0, 0], [0.01, 0, 0], [0, 0.01, 0]], F32), np.array([[0, 1, 2]], np.int64))
    for v, f in (tri, RC.tetrahedron()):
        for dtype in (torch.int32, torch.int64):
            for boundary in ('slide', 'pin'):
                gv, gf, gp, gm, info = _equal(dev, v, f, 0, dtype, boundary=boundary)
                assert np.array_equal(gf, f) and np.array_equal(RC._bits(gv), RC._bits(v)) and info['collapses'] == 0 and info['reached'] == (len(f) <= 1)


def check_cube_shape(dev):
    """issue item 2: 8 x 8 quads per side, 768 -> 48 faces"""
    v, f = cube(8)
    gv, gf, gp, gm, info = run(dev, v, f, 48)
    print(f'cube(8) 768 -> {len(gf)}: {info}, volume {volume(gv, gf)!r}')
    check_invariants(v, f, gv, gf, gp, gm, 48, closed=True)
    assert len(gf) == 48 and info['reached']
    corners = v[(np.abs(v) == 1).all(1)]
    have = {tuple(x) for x in RC._bits(gv[np.unique(gf)]).tolist()}
    assert len(corners) == 8 and all(tuple(x) in have for x in RC._bits(corners).tolist())
    used = gv[np.unique(gf)].astype(F64)
    assert np.all(np.abs(used).max(1) <= 1 + 1e-6) and np.all(np.abs(np.abs(used).max(1) - 1) <= 1e-6)                 # on the surface of [-1, 1]^3
    assert abs(volume(gv, gf) - 8.0) <= 1e-5


@functools.lru_cache(maxsize=None)
def quality_reference():
    v, f = lumpy_sphere()
    ref = greedy_yardstick(v, f, (320, 128))
    return {t: (rv, rf, rms_pair(v, f, rv, rf)) for t, (rv, rf) in ref.items()}


def _short_edge_route(dev, v, f, target):
    """collapse_short_edges driven to `target` faces: one round at a time, lo = the length below which just enough edges lie"""
    tv, tf, _ = RC._t(dev, v, f)
    for _ in range(400):
        nf = int(tf.shape[0])
        if nf <= target:
            break
        L = np.sort(RC._edge_lengths(tv.cpu().numpy(), tf.cpu().numpy()))
        lo = float(L[min((nf - target + 1) // 2, len(L) - 1)]) * (1 + 1e-6)
        nv, tf2, _, _ = MR.collapse_short_edges(tv, tf, lo, 1e9, rounds=1)
        if tf2.shape[0] == nf:
            break
        tv, tf = nv, tf2
    return tv.cpu().numpy(), tf.cpu().numpy()


def check_quality(dev, target):
    """issue item 3: both one-sided RMS distances <= 1.25 x the classic algorithm's and <= 0.5 x shortest-edge collapse's, at the same face count"""
    v, f = lumpy_sphere()
    gv, gf, gp, gm, info = run(dev, v, f, target)
    check_invariants(v, f, gv, gf, gp, gm, target, closed=True)
    rv, rf, ref = quality_reference()[target]
    got = rms_pair(v, f, gv, gf)
    sv, sf = _short_edge_route(dev, v, f, target)
    short = rms_pair(v, f, sv, sf)
    print(f'lumpy sphere 1280 -> {target}: {info}; faces: rounds {len(gf)}, classic {len(rf)}, shortest-edge {len(sf)}')
    print(f'  RMS (to the input, from the input): rounds {got}, classic {ref}, shortest-edge {short}')
    print(f'  ratio to classic {got[0] / ref[0]:.3f} / {got[1] / ref[1]:.3f}, to shortest-edge {got[0] / short[0]:.3f} / {got[1] / short[1]:.3f}')
    assert len(gf) == target and info['reached'] and len(rf) == target
    assert got[0] <= 1.25 * ref[0] and got[1] <= 1.25 * ref[1]
    assert got[0] <= 0.5 * short[0] and got[1] <= 0.5 * short[1]


def check_rejects(dev):
    v, f = RC.octahedron()
    tv, tf, _ = RC._t(dev, v, f)
    calls = []
    real = MR.L.call
    MR.L.call = lambda *a: calls.append(a)
    try:
        for x in (tv.double(), tv[:, :2], tv.reshape(-1)):
            with pytest.raises(RuntimeError, match='positions'):
                MR.decimate(x, tf, 4)
        for x in (tf.float(), tf[:, :2], tf.reshape(-1), tf.to(torch.int16)):
            with pytest.raises(RuntimeError, match='faces'):
                MR.decimate(tv, x, 4)
        for x in (torch.zeros(len(v) + 1, dtype=torch.bool, device=dev), torch.zeros(len(v), dtype=torch.float32, device=dev)):
            with pytest.raises(RuntimeError, match='pin_mask'):
                MR.decimate(tv, tf, 4, pin_mask=x)
        for x in (tf.clone().index_put_((torch.tensor(0), torch.tensor(0)), torch.tensor(len(v))), tf.clone().index_put_((torch.tensor(1), torch.tensor(2)), torch.tensor(-1))):
            with pytest.raises(RuntimeError, match='outside'):
                MR.decimate(tv, x, 4)
        with pytest.raises(RuntimeError, match='target_faces'):
            MR.decimate(tv, tf, -1)
        for bad in (0.0, -1.0, float('nan')):
            with pytest.raises(RuntimeError, match='window'):
                MR.decimate(tv, tf, 4, window=bad)
        with pytest.raises(RuntimeError, match='window'):
            MR.decimate(tv, tf, 4, min_window=0)
        with pytest.raises(RuntimeError, match='boundary'):
            MR.decimate(tv, tf, 4, boundary='move')
        for bad in (-1.0, float('nan')):
            with pytest.raises(RuntimeError, match='max_cost'):
                MR.decimate(tv, tf, 4, max_cost=bad)
    finally:
        MR.L.call = real
    assert not calls


# ---- the export chain ---------------------------------------------------------------------------------------------------------------------------
def check_lod_chain(dev, tmp_path):
    """issue item 6: icosphere(3), a small seeded MLPTexture3D, 256^2 maps, face_counts (1280, 320, 80)"""
    import os
    import texmat_cases as TC
    import uvatlas_cases as UC
    from d3h import export, uvatlas as UA
    from oracle import texmlp as OT
    from render import mesh as rmesh, mlptexture, util
    v, f = ico(3)
    tv = torch.as_tensor(v * F32(0.6), device=dev).contiguous()
    tf = torch.as_tensor(f, device=dev)
    R = 256
    torch.manual_seed(23)
    lo, hi = torch.tensor([0, 0, 0, 0, 0.001, 0.0], device=dev), torch.tensor([1, 1, 1, 0, 1.0, 1.0], device=dev)
    mlp = mlptexture.MLPTexture3D((tv.min(0).values, tv.max(0).values), channels=6, min_max=[lo, hi])
    with torch.no_grad():
        mlp.encoder.params.uniform_(-0.5, 0.5)
    mat = {'bsdf': 'pbr', 'kd_ks': mlp, 'name': 'fit'}
    base = rmesh.auto_normals(rmesh.Mesh(tv, tf, material=mat))
    ranges = ([0, 0, 0], [1, 1, 1], [0, 0.001, 0], [0, 1, 1], [-1, -1, 0], [1, 1, 1])
    counts = (1280, 320, 80)
    chain = export.lod_chain(base, mat, counts, R, *ranges)
    assert len(chain) == 3 and [int(m.t_pos_idx.shape[0]) for m in chain] == list(counts)
    assert torch.equal(chain[0].v_pos, tv) and torch.equal(chain[0].t_pos_idx, tf) and 'kd_ks' in mat
    cells = []
    w = [mlp.net.net[i].weight.detach().cpu() for i in (0, 2, 4)]
    for i, m in enumerate(chain):
        F = int(m.t_pos_idx.shape[0])
        A = UA.make_atlas(m.v_pos, m.t_pos_idx, (R, R))
        assert (A.s, A.nx, A.ny) == UC.yard_cell(F, R, R) and torch.equal(m.v_tex, A.uvs) and torch.equal(m.t_tex_idx, A.t_tex_idx)
        cells.append(A.s)
        pos, owned, _, _ = UA.bake_positions(A, m.v_pos, m.t_pos_idx)
        o = owned[0, ..., 0] > 0
        got = torch.cat((m.material['kd'].data, m.material['ks'].data), -1).detach()[0]

        def ref(dtype):
            x = pos[0][o].cpu().to(dtype)
            b0, b1 = torch.tensor(mlp.BBOX[:3], dtype=dtype), torch.tensor(mlp.BBOX[3:], dtype=dtype)
            e = OT.grid_encode(torch.clamp((x - b0) / (b1 - b0), 0, 1), mlp.encoder.params.detach().cpu().to(dtype))
            h = torch.relu(torch.relu(e @ w[0].to(dtype).T) @ w[1].to(dtype).T) @ w[2].to(dtype).T
            return torch.sigmoid(h) * (hi.cpu().to(dtype) - lo.cpu().to(dtype)) + lo.cpu().to(dtype)
        with torch.no_grad():
            UC.assert_close(f'level {i} ({F} faces, s = {A.s}): kd / ks on owned texels vs the network at its own surface', got[o].cpu(), ref(torch.float64),
                            ref(torch.float32))
        assert bool((m.material['normal'].data == torch.tensor([0.0, 0.0, 1.0], device=dev)).all()) and m.v_nrm is not None
    print('cell sizes down the chain', cells)
    assert cells[0] < cells[1] < cells[2]
    folders = export.write_lod_chain(str(tmp_path), chain)
    assert folders == [os.path.join(str(tmp_path), f'lod{i}') for i in range(3)]
    _, _, mvp, cam, draws = TC._scene_np()
    mvp, cam = mvp.to(dev), cam.to(dev)
    q = lambda x: torch.round(255 * x) / 255
    with torch.no_grad():
        for i, (m, folder) in enumerate(zip(chain, folders)):
            assert sorted(os.listdir(folder)) == ['mesh.mtl', 'mesh.obj', 'texture_kd.png', 'texture_ks.png', 'texture_n.png']
            back = export.load_textured_mesh(os.path.join(folder, 'mesh.obj'), device=dev)
            assert torch.equal(back.t_pos_idx.long(), m.t_pos_idx.long()) and torch.equal(back.t_tex_idx.long(), m.t_tex_idx.long())
            assert float((back.v_pos - m.v_pos).abs().max()) <= 1e-6                                                  # positions pass through text
            kd, ks = m.material['kd'].data.detach(), m.material['ks'].data.detach()
            assert float((back.material['kd'].data.to(dev) - util.srgb_to_rgb(q(util.rgb_to_srgb(kd)))).abs().max()) <= 1e-6     # the PNG's 8 bits
            assert float((back.material['ks'].data.to(dev) - q(ks)).abs().max()) <= 1e-6
            out = TC.render(rmesh.compute_tangents(m), None, mvp, cam, draws, buffers=('shaded', 'kd'))
            cover = out['kd'][..., 3] > 0 if out['kd'].shape[-1] == 4 else out['kd'].abs().sum(-1) > 0
            print(f'level {i}: rendered, {int(cover.sum())} pixels covered')
            assert bool(torch.isfinite(out['shaded']).all()) and int(cover.sum()) > 100
            again = TC.render(back, None, mvp, cam, draws, buffers=('kd',))
            assert bool(torch.isfinite(again['kd']).all())
    with pytest.raises(ValueError, match='face_counts'):
        export.lod_chain(base, mat, (1280, 1280), R, *ranges)
    with pytest.raises(ValueError, match='face_counts'):
        export.lod_chain(base, mat, (320, 640), R, *ranges)
    with pytest.raises(ValueError, match='face_counts'):
        export.lod_chain(base, mat, (), R, *ranges)
    with pytest.raises(ValueError, match='texture_res'):
        export.lod_chain(base, mat, counts, [R, R, R, R], *ranges)
    with pytest.raises(ValueError, match='volumetric'):
        export.lod_chain(chain[0], chain[0].material, counts, R, *ranges)
    two = export.lod_chain(base, mat, (1280, 640), [160, (96, 128)], *ranges)
    assert two[0].material['kd'].data.shape == (1, 160, 160, 3) and two[1].material['kd'].data.shape == (1, 96, 128, 3) and two[1].t_pos_idx.shape[0] == 640
