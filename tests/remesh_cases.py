"""Check functions of the collapse, flip, smoothing and reprojection steps of isotropic remeshing (csrc/meshremesh.hip, d3h/meshrefine.py), shared by
tests/test_remesh_emul.py (host emulation of the kernel sources) and tests/test_gpu_remesh.py (MI355X).  Same shapes on both.  Every mesh is generated
here from a seed.

Yardsticks:
  collapse, flip   a sequential numpy restatement of the docstring of d3h.meshrefine in float32, every operation rounded once in the stated order.
                   Selection is a minimum over sets, so the restatement has no notion of parallelism.  EXACT: faces, parent, vmap and the flip count
                   as integers, positions bit for bit.  (A collapse's link, length and normal checks belong to candidacy, as the docstring says.)
  smooth           the same rules one vertex at a time in float64, and in float32 for the parity rule's own error (optixutils_cases.assert_close).
                   A vertex whose float64 rejection test or normal length is borderline (relative margin < 1e-5) is left out; their share is
                   asserted <= 1 % from the float64 side alone, before the kernel runs.
  reproject        the closest point over ALL input triangles in float64 (Ericson's region test), same parity rule; a vertex with two near-equal
                   nearest triangles (squared distances within 1e-5 relative) whose closest points differ is left out, share <= 1 %.
  isotropic_remesh the restatement of the whole loop (float32 rules, float64 brute-force reprojection rounded to float32).  The chain is not compared
                   bit for bit (the BVH's barycentrics are not the yardstick's), so the invariants and the quality figures are asserted on the
                   restatement AND on the result of the code under test.
The emulator runs the threads of a launch one after another, so it cannot show a race: the contended cases count on the GPU."""
import functools
import os
import types

import numpy as np
import pytest
import torch

import handoff_cases as HC
import optixutils_cases as OC
from d3h import meshrefine as MR
from d3h import raytrace as RT

F32 = np.float32
MAXKEY = np.uint64(0xffffffffffffffff)


# ---- mesh generators ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _icosphere(level):
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6),
         (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(p, np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(level):
        mid, out = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[k] = len(v) - 1
            return mid[k]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = out
    return np.array(v), np.array(f, np.int64)


@functools.lru_cache(maxsize=None)
def sphere_case(open_cap):
    """icosphere(3), 1280 faces, radius 0.8, tangential jitter sigma = 0.02 (re-projected to the sphere); open: the cap z > 0.6 removed"""
    v, f = _icosphere(3)
    rng = np.random.default_rng(20241)
    j = rng.normal(0.0, 0.02, v.shape)
    j -= v * (j * v).sum(1, keepdims=True)
    p = v * 0.8 + j
    p *= 0.8 / np.linalg.norm(p, axis=1, keepdims=True)
    if open_cap:
        f = f[~(p[f][:, :, 2] > 0.6).all(1)]
    return p.astype(F32), f


def tetrahedron():
    v, f = HC.tetrahedron()
    return (v * 0.05).astype(F32), f


def octahedron():
    v = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float64) * 0.05
    f = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], np.int64)
    return v.astype(F32), f


def fin():
    """three triangles on one edge: non-manifold, every vertex pinned"""
    v = np.array([[0, 0, 0], [0.01, 0, 0], [0, 0.01, 0], [0, -0.01, 0], [0, 0, 0.01]], F32)
    return v, np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4]], np.int64)


def short_strip(k):
    """a band of three rows, k columns of pitch 0.1 in x with every second column 0.03 after the one before: the middle row's short edges all have the
    SAME float32 length class by construction of the columns (ties go by rank), the outer rows are boundary and pinned"""
    xs = np.cumsum([0.0] + [0.03 if i % 2 == 0 else 0.1 for i in range(k)])
    v = np.array([[x, y, 0.0] for y in (0.0, 0.1, 0.2) for x in xs], F32)
    w = len(xs)
    f = []
    for r in range(2):
        for i in range(w - 1):
            a, b = r * w + i, r * w + i + 1
            f += [(a, b, b + w), (a, b + w, a + w)]
    return v, np.array(f, np.int64)


def dented_sheet(k):
    """a W x H sheet of pitch 1 (diagonals (x,y)-(x+1,y+1)) in which k interior vertices are pulled 0.6 towards their +x neighbour: exactly k edges shorter
    than 0.5.  The pulled vertices stand 3 apart in x and 2 in y, so their closed neighbourhoods overlap and claims contend."""
    per_row = 20
    W, H = 3 * per_row + 2, 2 * ((k + per_row - 1) // per_row) + 2
    v = np.array([[x, y, 0.0] for y in range(H) for x in range(W)], np.float64)
    rng = np.random.default_rng(77 + k)
    v[:, 2] = rng.normal(0.0, 0.01, len(v))
    done = 0
    for y in range(1, H - 1, 2):
        for x in range(1, W - 2, 3):
            if done < k:
                v[y * W + x, 0] += 0.6 + 0.001 * rng.uniform(-1, 1)
                done += 1
    assert done == k
    f = []
    for y in range(H - 1):
        for x in range(W - 1):
            a = y * W + x
            f += [(a, a + 1, a + W + 1), (a, a + W + 1, a + W)]
    return v.astype(F32), np.array(f, np.int64)


# ---- the restatement --------------------------------------------------------------------------------------------------------------------------
def _dot(u, w):
    return (u[..., 0] * w[..., 0] + u[..., 1] * w[..., 1]) + u[..., 2] * w[..., 2]


def _cross(u, w):
    return np.stack([u[..., 1] * w[..., 2] - u[..., 2] * w[..., 1], u[..., 2] * w[..., 0] - u[..., 0] * w[..., 2], u[..., 0] * w[..., 1] - u[..., 1] * w[..., 0]], -1)


def _nrm(p0, p1, p2):
    return _cross(p1 - p0, p2 - p0)


def _len2(a, b):
    d = b - a
    return _dot(d, d)


def _cos_ok(n, m, c2):
    d = _dot(n, m)
    return (d > 0) & (d * d >= c2 * (_dot(n, n) * _dot(m, m)))


class Adjacency:
    def __init__(self, f, n, pin):
        f = np.asarray(f, np.int64).reshape(-1, 3)
        a, b = f.reshape(-1), f[:, [1, 2, 0]].reshape(-1)
        keys, cnt = np.unique((np.minimum(a, b) << 32) | np.maximum(a, b), return_counts=True)
        self.elo, self.ehi, self.cnt = keys >> 32, keys & 0xffffffff, cnt
        self.edge_set = set(keys.tolist())
        nb, vf = [set() for _ in range(n)], [set() for _ in range(n)]
        for lo, hi in zip(self.elo.tolist(), self.ehi.tolist()):
            if lo != hi:
                nb[lo].add(hi)
                nb[hi].add(lo)
        for fi, row in enumerate(f.tolist()):
            for i in row:
                vf[i].add(fi)
        self.nbr, self.vf = [sorted(s) for s in nb], [sorted(s) for s in vf]
        self.val = np.array([len(s) for s in nb], np.int64)
        pinned = np.zeros(n, bool) if pin is None else np.asarray(pin, bool).copy()
        odd = cnt != 2
        pinned[self.elo[odd]] = True
        pinned[self.ehi[odd]] = True
        self.pinned = pinned


def _select(n, cands, keys, claim_sets):
    claim = np.full(n, MAXKEY, np.uint64)
    for r, s in zip(cands, claim_sets):
        for x in s:
            claim[x] = min(claim[x], keys[r])
    return [r for r, s in zip(cands, claim_sets) if all(claim[x] == keys[r] for x in s)]


def collapse_round_yardstick(v, f, lo, hi, pin, stats=None):
    """-> None when nothing collapses, else (v', f', parent, vmap, keep)"""
    n = len(v)
    A = Adjacency(f, n, pin)
    lo2, hi2 = F32(lo) * F32(lo), F32(hi) * F32(hi)
    l2 = _len2(v[A.elo], v[A.ehi])
    assert l2.dtype == np.float32
    cand = (A.cnt == 2) & (A.elo != A.ehi) & ~(A.pinned[A.elo] & A.pinned[A.ehi]) & (l2 < lo2)
    keys = (l2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(len(l2), dtype=np.uint64)
    def checks(r):
        """-> (q, survivor, removed) when the link, length and normal checks pass, else None"""
        a, b = int(A.elo[r]), int(A.ehi[r])
        common = sorted(set(A.nbr[a]) & set(A.nbr[b]))
        if len(common) != 2 or any(A.val[x] <= 3 for x in common):
            return None
        pa, pb = A.pinned[a], A.pinned[b]
        q = v[a] if pa else (v[b] if pb else (v[a] + v[b]) * F32(0.5))
        ring = [x for x in A.nbr[a] if x != b] + [x for x in A.nbr[b] if x != a]
        if not all(_len2(q, v[x]) <= hi2 for x in ring):
            return None
        for end, other in ((a, b), (b, a)):
            for fi in A.vf[end]:
                row = [int(i) for i in f[fi]]
                if other in row:
                    continue
                if not _cos_ok(_nrm(*[v[i] for i in row]), _nrm(*[q if i == end else v[i] for i in row]), F32(0.25)):
                    return None
        return (q, b, a) if pb else (q, a, b)

    passed = {r: checks(r) for r in np.nonzero(cand)[0].tolist()}
    cands = [r for r in passed if passed[r] is not None]
    sets = [{int(A.elo[r]), int(A.ehi[r])} | set(A.nbr[A.elo[r]]) | set(A.nbr[A.ehi[r]]) for r in cands]
    selected = _select(n, cands, keys, sets)
    if stats is not None:
        stats.append((len(cands), len(selected)))
    vout, remap, drop, done = v.copy(), np.arange(n), np.zeros(len(f), bool), 0
    for r in selected:
        q, s_, o = passed[r]
        vout[s_] = q
        remap[o] = s_
        for fi in A.vf[s_]:
            if o in f[fi]:
                drop[fi] = True
        done += 1
    if done == 0:
        return None
    keep = remap == np.arange(n)
    newidx = np.cumsum(keep) - 1
    return vout[keep], newidx[remap[f[~drop]]], np.nonzero(~drop)[0], newidx[remap], keep


def collapse_yardstick(v, f, lo, hi, rounds=8, pin=None, stats=None):
    v, f = np.asarray(v, F32), np.asarray(f, np.int64).reshape(-1, 3)
    parent, vmap, src = np.arange(len(f)), np.arange(len(v)), np.arange(len(v))
    pin = None if pin is None else np.asarray(pin, bool)
    for _ in range(rounds):
        if len(f) == 0:
            break
        r = collapse_round_yardstick(v, f, lo, hi, pin, stats)
        if r is None:
            break
        v, f, p, m, keep = r
        parent, vmap, src = parent[p], m[vmap], src[keep]
        pin = None if pin is None else pin[keep]
    return v, f, parent, vmap, pin, src


def flip_round_yardstick(v, f, pin, stats=None):
    """flips in place, -> the number of flips"""
    n = len(v)
    A = Adjacency(f, n, pin)
    directed = {}
    for fi, (i0, i1, i2) in enumerate(f.tolist()):
        for x, y, z in ((i0, i1, i2), (i1, i2, i0), (i2, i0, i1)):
            directed.setdefault((x, y), []).append((fi, z))
    rows = []
    for r, (a, b, c2) in enumerate(zip(A.elo.tolist(), A.ehi.tolist(), A.cnt.tolist())):
        if c2 != 2 or a == b:
            continue
        ab, ba = directed.get((a, b), []), directed.get((b, a), [])
        if len(ab) != 1 or len(ba) != 1:
            continue
        (fab, c), (fba, d) = ab[0], ba[0]
        if fab == fba or c == d or len({a, b, c, d}) != 4 or ((min(c, d) << 32) | max(c, d)) in A.edge_set:
            continue
        tgt = [4 if A.pinned[x] else 6 for x in (a, b, c, d)]
        val = [int(A.val[x]) for x in (a, b, c, d)]
        gain = sum(abs(x - t) for x, t in zip(val, tgt)) - sum(abs(x + s - t) for x, s, t in zip(val, (-1, -1, 1, 1), tgt))
        if gain > 0:
            rows.append((r, a, b, c, d, fab, fba, gain))
    if not rows:
        return 0
    R = np.array(rows, np.int64)
    P, Q, C, D = v[R[:, 1]], v[R[:, 2]], v[R[:, 3]], v[R[:, 4]]
    n1, n2, m1, m2 = _nrm(P, Q, C), _nrm(Q, P, D), _nrm(P, D, C), _nrm(D, Q, C)
    assert n1.dtype == np.float32
    ok = _cos_ok(n1, n2, F32(0.75)) & _cos_ok(m1, n1, F32(0.25)) & _cos_ok(m1, n2, F32(0.25)) & _cos_ok(m2, n1, F32(0.25)) & _cos_ok(m2, n2, F32(0.25))
    R = R[ok]
    keys = {int(r): (np.uint64(15 - min(int(g), 15)) << np.uint64(32)) | np.uint64(r) for r, g in zip(R[:, 0], R[:, 7])}
    cands = [int(r) for r in R[:, 0]]
    sets = [set(row[1:5].tolist()) for row in R]
    selected = set(_select(n, cands, keys, sets))
    if stats is not None:
        stats.append((len(cands), len(selected)))
    for r, a, b, c, d, fab, fba, _ in R.tolist():
        if r in selected:
            f[fab] = (a, d, c)
            f[fba] = (d, b, c)
    return len(selected)


def flip_yardstick(v, f, rounds=8, pin=None, stats=None):
    v, f = np.asarray(v, F32), np.array(f, np.int64).reshape(-1, 3)
    total = 0
    for _ in range(rounds):
        if len(f) == 0:
            break
        k = flip_round_yardstick(v, f, pin, stats)
        if k == 0:
            break
        total += k
    return f, total


def smooth_yardstick(v, f, pin=None, dtype=np.float64):
    """-> (v', margin [n]): the smallest relative margin of the decisions taken for each vertex (inf where none is taken)"""
    v = np.asarray(v, F32).astype(dtype)
    f = np.asarray(f, np.int64).reshape(-1, 3)
    A = Adjacency(f, len(v), pin)
    out, margin = v.copy(), np.full(len(v), np.inf)
    one = dtype(1.0)
    for i in range(len(v)):
        if A.pinned[i] or not A.nbr[i]:
            continue
        g = np.zeros(3, dtype)
        for j in A.nbr[i]:
            g = g + v[j]
        g = g * (one / dtype(len(A.nbr[i])))
        nsum = np.zeros(3, dtype)
        for fi in A.vf[i]:
            nsum = nsum + _nrm(*v[f[fi]])
        nn = _dot(nsum, nsum)
        scale = sum(float(_dot(_nrm(*v[f[fi]]), _nrm(*v[f[fi]]))) for fi in A.vf[i])
        margin[i] = float(nn) / max(scale, 1e-300)
        if not nn > 0:
            continue
        nsum = nsum / np.sqrt(nn)
        d = g - v[i]
        t = _dot(nsum, d)
        q = (v[i] + d) - nsum * t
        ok = True
        for fi in A.vf[i]:
            p = v[f[fi]]
            pn = np.where((f[fi] == i)[:, None], q[None], p)
            old, new = _nrm(*p), _nrm(*pn)
            dd = _dot(new, old)
            margin[i] = min(margin[i], abs(float(dd)) / max(float(np.sqrt(_dot(new, new) * _dot(old, old))), 1e-300))
            ok = ok and bool(dd > 0)
        if ok:
            out[i] = q
    return out, margin


def closest_points(p, v0, f0, dtype=np.float64):
    """-> (point [m,3], borderline [m]): the closest point of the triangle soup to each p (Ericson, Real-Time Collision Detection 5.1.5), all triangles"""
    p, v0 = np.asarray(p, dtype), np.asarray(v0, dtype)
    A, B, C = v0[f0[:, 0]][None], v0[f0[:, 1]][None], v0[f0[:, 2]][None]
    P = p[:, None]
    ab, ac, ap = B - A, C - A, P - A
    d1, d2 = (ab * ap).sum(-1), (ac * ap).sum(-1)
    bp = P - B
    d3, d4 = (ab * bp).sum(-1), (ac * bp).sum(-1)
    cp = P - C
    d5, d6 = (ab * cp).sum(-1), (ac * cp).sum(-1)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    with np.errstate(divide='ignore', invalid='ignore'):
        den = va + vb + vc
        bv, bw = vb / den, vc / den
        cands = [
            (np.ones_like(d1, bool), 0 * d1 + 1 - bv - bw, bv, bw),
            ((va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0), 0 * d1, 1 - (d4 - d3) / ((d4 - d3) + (d5 - d6)), (d4 - d3) / ((d4 - d3) + (d5 - d6))),
            ((vb <= 0) & (d2 >= 0) & (d6 <= 0), 1 - d2 / (d2 - d6), 0 * d1, d2 / (d2 - d6)),
            ((d6 >= 0) & (d5 <= d6), 0 * d1, 0 * d1, 0 * d1 + 1),
            ((vc <= 0) & (d1 >= 0) & (d3 <= 0), 1 - d1 / (d1 - d3), d1 / (d1 - d3), 0 * d1),
            ((d3 >= 0) & (d4 <= d3), 0 * d1, 0 * d1 + 1, 0 * d1),
            ((d1 <= 0) & (d2 <= 0), 0 * d1 + 1, 0 * d1, 0 * d1)]
    b0, b1, b2 = cands[0][1:]
    for m, x, y, z in cands[1:]:                        # later entries take precedence: the order of Ericson's early returns, reversed
        b0, b1, b2 = np.where(m, x, b0), np.where(m, y, b1), np.where(m, z, b2)
    pts = (b0[..., None] * A + b1[..., None] * B) + b2[..., None] * C
    dist2 = ((pts - P) ** 2).sum(-1)
    dist2 = np.where(np.isfinite(dist2), dist2, np.inf)
    best = dist2.argmin(1)
    rows = np.arange(len(p))
    bp_, bd = pts[rows, best], dist2[rows, best]
    near = dist2 <= bd[:, None] * (1 + 1e-5) + 1e-30
    spread = np.where(near[..., None], np.abs(pts - bp_[:, None]), 0).max((1, 2))
    return bp_, spread > 1e-6 * np.abs(v0).max()


def isotropic_yardstick(v, f, t, iterations=3, pin=None, reproject=True, log=None):
    v0, f0 = np.asarray(v, F32), np.asarray(f, np.int64).reshape(-1, 3)
    v, f = v0, f0
    parent = np.arange(len(f))
    hi, lo = t * 4.0 / 3.0, t * 4.0 / 5.0
    pin = None if pin is None else np.asarray(pin, bool)
    for _ in range(iterations):
        n = len(v)
        v, f, p, _ = HC.refine_yardstick(v, f, hi, 1)
        parent = parent[p]
        moved = np.zeros(len(v), bool)
        moved[n:] = True
        if pin is not None:
            pin = np.concatenate([pin, np.zeros(len(v) - n, bool)])
        cs, fs = [], []
        vc, f, p, vmap, pin, src = collapse_yardstick(v, f, lo, hi, 8, pin, cs)
        parent = parent[p]
        carried = np.zeros(len(vc), bool)
        np.logical_or.at(carried, vmap, moved)
        moved = carried | (vc != v[src]).any(1)
        f, _ = flip_yardstick(vc, f, 8, pin, fs)
        v = smooth_yardstick(vc, f, pin, F32)[0]
        moved |= (v != vc).any(1)
        if reproject and moved.any():
            v = v.copy()
            v[moved] = closest_points(v[moved], v0, f0)[0].astype(F32)
        if log is not None:
            log.append((len(v) - 0, len(f), [c[1] for c in cs], [c[1] for c in fs]))
    return v, f, parent


# ---- invariants and figures, float64, from the returned arrays alone -----------------------------------------------------------------------------
def _edge_lengths(v, f):
    e = HC._edges(f)[0]
    e = e[e[:, 0] != e[:, 1]]
    v = np.asarray(v, np.float64)
    return np.linalg.norm(v[e[:, 0]] - v[e[:, 1]], axis=1)


def _boundary(v, f):
    e, c = HC._edges(f)
    return sorted(tuple(sorted((tuple(np.asarray(v, F32)[a].view(np.uint32).tolist()), tuple(np.asarray(v, F32)[b].view(np.uint32).tolist())))) for a, b in e[c == 1])


def check_invariants(v0, f0, v1, f1, parent=None, vmap=None, pin=None, hi=None, closed=False):
    v0, v1, f0, f1 = np.asarray(v0, F32), np.asarray(v1, F32), np.asarray(f0, np.int64), np.asarray(f1, np.int64)
    assert f1.min() >= 0 and f1.max() < len(v1)
    assert np.all((f1[:, 0] != f1[:, 1]) & (f1[:, 1] != f1[:, 2]) & (f1[:, 2] != f1[:, 0]))                         # no repeated index
    c0, c1 = HC._edges(f0)[1], HC._edges(f1)[1]
    assert c1.max() <= max(2, c0.max()) and (c1 == 1).sum() == (c0 == 1).sum() and (c1 > 2).sum() == (c0 > 2).sum()
    assert HC._euler(f1) == HC._euler(f0)
    assert _boundary(v1, f1) == _boundary(v0, f0)                                                                    # boundary edges bit-unchanged
    if closed:
        assert np.all(c1 == 2) and HC._signed_volume(v1.astype(np.float64), f1) * HC._signed_volume(v0.astype(np.float64), f0) > 0
    if parent is not None:
        assert len(parent) == len(f1) and np.all(np.diff(parent) >= 0) and parent.min() >= 0 and parent.max() < len(f0)
    if vmap is not None:
        pinned = Adjacency(f0, len(v0), pin).pinned
        assert len(vmap) == len(v0) and vmap.min() >= 0 and vmap.max() < len(v1)
        assert np.array_equal(v1[vmap[pinned]].view(np.uint32), v0[pinned].view(np.uint32))                         # pinned: still there, not moved
        first = np.full(len(v1), len(v0))
        np.minimum.at(first, vmap, np.arange(len(v0)))
        assert np.all(first < len(v0)) and np.all(np.diff(first) > 0)                                                # survivors keep their order
    if hi is not None:
        old = _edge_lengths(v0, f0).max()
        assert _edge_lengths(v1, f1).max() <= max(old, float(F32(hi)) * (1 + 1e-6))                                  # a collapse creates no edge longer than hi


def figures(v, f, t):
    L = _edge_lengths(v, f)
    val = np.bincount(HC._edges(f)[0].reshape(-1))
    return dict(short=float((L < 0.8 * t).mean()), long=float((L > 4.0 / 3.0 * t).mean()), min_edge=float(L.min()), val6=float((val[val > 0] == 6).mean()),
                nv=int(len(np.unique(f))), nf=int(len(f)))


# ---- drivers of the code under test -----------------------------------------------------------------------------------------------------------
def _t(dev, v, f, dtype=torch.int64, pin=None):
    return (torch.as_tensor(np.asarray(v, F32), device=dev), torch.as_tensor(np.asarray(f), dtype=dtype, device=dev).reshape(-1, 3),
            None if pin is None else torch.as_tensor(np.asarray(pin, bool), device=dev))


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _collapse_equal(dev, v, f, lo, hi, rounds=8, pin=None, dtype=torch.int64, stats=None):
    yv, yf, yp, ym, _, _ = collapse_yardstick(v, f, lo, hi, rounds, pin, stats)
    tv, tf, tp = _t(dev, v, f, dtype, pin)
    gv, gf, gp, gm = MR.collapse_short_edges(tv, tf, lo, hi, rounds, tp)
    assert gf.dtype == dtype and gp.dtype == torch.int64 and gm.dtype == torch.int64 and gv.dtype == torch.float32
    gv, gf, gp, gm = gv.cpu().numpy(), gf.cpu().numpy().astype(np.int64), gp.cpu().numpy(), gm.cpu().numpy()
    assert gf.shape == yf.shape and np.array_equal(gf, yf)
    assert np.array_equal(gp, yp) and np.array_equal(gm, ym)
    assert gv.shape == yv.shape and np.array_equal(_bits(gv), _bits(yv))
    return gv, gf, gp, gm


def _flip_equal(dev, v, f, rounds=8, pin=None, dtype=torch.int64, stats=None):
    yf, yn = flip_yardstick(v, f, rounds, pin, stats)
    tv, tf, tp = _t(dev, v, f, dtype, pin)
    gf, gn = MR.flip_edges(tv, tf, rounds, tp)
    assert gf.dtype == dtype and gn == yn, (gn, yn)
    gf = gf.cpu().numpy().astype(np.int64)
    assert np.array_equal(gf, yf)
    assert np.array_equal(tf.cpu().numpy(), np.asarray(f).reshape(-1, 3))                                             # the input is not written
    return gf, gn


def _smooth_close(dev, what, v, f, pin=None, dtype=torch.int64):
    r64, margin = smooth_yardstick(v, f, pin, np.float64)
    r32, _ = smooth_yardstick(v, f, pin, F32)
    sure = margin >= 1e-5
    print(f'{what}: {(~sure).sum()} of {len(sure)} vertices borderline')
    assert (~sure).mean() <= 0.01
    tv, tf, tp = _t(dev, v, f, dtype, pin)
    g = MR.smooth_tangential(tv, tf, tp).cpu().numpy()
    pinned = Adjacency(f, len(v), pin).pinned
    assert np.array_equal(_bits(g[pinned]), _bits(np.asarray(v, F32)[pinned]))
    moved = (r64 != np.asarray(v, F32).astype(np.float64)).any(1)
    assert np.array_equal(_bits(g[sure & ~moved]), _bits(np.asarray(v, F32)[sure & ~moved]))                         # rejected or without neighbours: the same bits
    OC.assert_close(what, g[sure], r64[sure], r32[sure].astype(np.float64))
    return g


# ---- checks ---------------------------------------------------------------------------------------------------------------------------------------
def check_small(dev):
    """F = 0, everything pinned, tetrahedron / octahedron (link rule), a fin, unreferenced vertices: unchanged where the rules say so, exact always"""
    v = np.zeros((3, 3), F32)
    tv, tf, _ = _t(dev, v, np.zeros((0, 3), np.int64))
    gv, gf, gp, gm = MR.collapse_short_edges(tv, tf, 1.0, 2.0)
    assert gv.shape == (3, 3) and gf.shape == (0, 3) and gp.shape == (0,) and np.array_equal(gm.cpu().numpy(), np.arange(3))
    assert MR.flip_edges(tv, tf)[0].shape == (0, 3) and MR.flip_edges(tv, tf)[1] == 0
    assert torch.equal(MR.smooth_tangential(tv, tf), tv)
    iv, if_, ip = MR.isotropic_remesh(tv, tf, 0.1)
    assert torch.equal(iv, tv) and if_.shape == (0, 3) and ip.shape == (0,)
    tri = (np.array([[0, 0, 0], [0.01, 0, 0], [0, 0.01, 0]], F32), np.array([[0, 1, 2]], np.int64))
    two = (np.array([[0, 0, 0], [0.01, 0, 0], [0, 0.01, 0], [0.01, 0.01, 0.002]], F32), np.array([[0, 1, 2], [2, 1, 3]], np.int64))
    lone = (np.concatenate([np.full((2, 3), 5.0, F32), octahedron()[0], np.full((1, 3), 7.0, F32)]), octahedron()[1] + 2)
    for name, (v, f), unchanged in (('triangle', tri, True), ('two triangles', two, True), ('fin', fin(), True), ('tetrahedron', tetrahedron(), True),
                                    ('octahedron', octahedron(), False), ('unreferenced', lone, False)):
        for dtype in (torch.int32, torch.int64):
            gv, gf, gp, gm = _collapse_equal(dev, v, f, 1.0, 2.0, dtype=dtype)                                      # every edge is shorter than lo
            ff, nflip = _flip_equal(dev, v, f, dtype=dtype)
            sm = _smooth_close(dev, name, v, f, dtype=dtype)
            if unchanged:
                assert np.array_equal(gf, f) and np.array_equal(_bits(gv), _bits(v)) and np.array_equal(gm, np.arange(len(v))) and nflip == 0
            if name in ('triangle', 'two triangles', 'fin'):
                assert np.array_equal(_bits(sm), _bits(v))                                                           # everything pinned
            if name in ('tetrahedron', 'octahedron', 'unreferenced'):
                assert np.all(HC._edges(gf)[1] == 2) and len(gf) >= 4                                                # closed stays closed: no two-faced fin
            assert np.all((gf[:, 0] != gf[:, 1]) & (gf[:, 1] != gf[:, 2]) & (gf[:, 2] != gf[:, 0])) and HC._euler(gf) == HC._euler(f)
        if name == 'unreferenced':
            assert len(gv) >= 3 and np.array_equal(gv[:2], lone[0][:2]) and np.array_equal(gv[-1], lone[0][-1])      # unreferenced vertices stay


def check_strip(dev, dtype):
    """equal-length short edges in a row: ties go by rank, neighbouring claims contend; the outer rows are boundary and stay"""
    v, f = short_strip(24)
    stats = []
    gv, gf, gp, gm = _collapse_equal(dev, v, f, 0.05, 0.25, dtype=dtype, stats=stats)
    print('strip: (candidates, selected) per round', stats)
    assert stats[0][0] >= 6 and 0 < stats[0][1] < stats[0][0] and len(gv) < len(v)                                  # claims contended: fewer selected than candidates
    check_invariants(v, f, gv, gf, gp, gm, hi=0.25)
    l2 = _len2(v[:, None], v[None])
    short = np.unique(l2[(l2 < F32(0.05) ** 2) & (l2 > 0)])
    assert len(short) < 12                                                                                           # there ARE ties among the keys' length bits


@functools.lru_cache(maxsize=None)
def _sheet(k):
    return dented_sheet(k)


def check_sheet(dev, k, dtype=torch.int64):
    """exactly k candidates (64 / 65: a wave's edge; 300: a workgroup's)"""
    v, f = _sheet(k)
    stats = []
    gv, gf, gp, gm = _collapse_equal(dev, v, f, 0.5, 2.5, dtype=dtype, stats=stats)
    print(f'sheet {k}: (candidates, selected) per round', stats)
    assert stats[0][0] == k and stats[0][1] > 0 and len(gv) < len(v)
    check_invariants(v, f, gv, gf, gp, gm, hi=2.5)
    ff, nflip = _flip_equal(dev, gv, gf, dtype=dtype)
    check_invariants(gv, gf, gv, ff)
    print(f'sheet {k}: {len(v) - len(gv)} collapses, then {nflip} flips')


def check_pin_mask(dev):
    v, f = _sheet(65)
    rng = np.random.default_rng(5)
    pin = rng.random(len(v)) < 0.3
    gv, gf, gp, gm = _collapse_equal(dev, v, f, 0.5, 2.5, pin=pin)
    check_invariants(v, f, gv, gf, gp, gm, pin=pin, hi=2.5)
    free = _collapse_equal(dev, v, f, 0.5, 2.5)
    assert len(free[0]) < len(gv) < len(v)                                                                           # the mask holds some back, not all
    sv, sf = sphere_case(False)
    pin = np.random.default_rng(6).random(len(sv)) < 0.3
    ff, n_pin = _flip_equal(dev, sv, sf, pin=pin)
    assert n_pin != _flip_equal(dev, sv, sf)[1]                                                                      # tgt = 4 at a pinned vertex changes the gains
    g = _smooth_close(dev, 'sphere, pin_mask', sv, sf, pin=pin)
    assert np.array_equal(_bits(g[pin]), _bits(sv[pin])) and not np.array_equal(g[~pin], sv[~pin])


def check_sphere_steps(dev, open_cap):
    v, f = sphere_case(open_cap)
    t = 0.2 if open_cap else 0.12
    lo, hi = 0.8 * t, 4.0 / 3.0 * t
    v, f, _, _ = HC.refine_yardstick(v, f, hi, 1)                       # as in the loop: a collapse must not make an edge longer than hi, so the long ones go first
    for dtype in (torch.int32, torch.int64):
        cs, fs = [], []
        gv, gf, gp, gm = _collapse_equal(dev, v, f, lo, hi, dtype=dtype, stats=cs)
        check_invariants(v, f, gv, gf, gp, gm, hi=hi, closed=not open_cap)
        ff, nflip = _flip_equal(dev, gv, gf, dtype=dtype, stats=fs)
        check_invariants(gv, gf, gv, ff, closed=not open_cap)
        sm = _smooth_close(dev, f'sphere open={open_cap}', gv, ff, dtype=dtype)
        check_invariants(gv, ff, sm, ff, closed=not open_cap)
    print(f'sphere open={open_cap}: collapse (candidates, selected) per round {cs}; flip {fs}; {len(v) - len(gv)} vertices removed, {nflip} flips')
    assert len(gv) < len(v) and nflip > 0 and len(cs) > 1 and cs[0][0] > 64


def check_reproject(dev):
    """the reprojection rule on its own: smoothed vertices of the jittered sphere back onto the input"""
    v, f = sphere_case(False)
    sm = smooth_yardstick(v, f, None, F32)[0]
    at = np.nonzero((sm != v).any(1))[0]
    r64, border = closest_points(sm[at], v, f, np.float64)
    r32, _ = closest_points(sm[at], v, f, F32)
    print(f'reproject: {border.sum()} of {len(at)} vertices borderline')
    assert border.mean() <= 0.01 and len(at) > 600
    tv, tf, _ = _t(dev, v, f)
    ts = torch.as_tensor(sm, device=dev)
    g = MR._reproject(ts, torch.as_tensor(at, device=dev), RT.Bvh(tv, tf), tv, tf.long()).cpu().numpy()
    others = np.setdiff1d(np.arange(len(v)), at)
    assert np.array_equal(_bits(g[others]), _bits(sm[others]))
    OC.assert_close('reprojected positions', g[at][~border], r64[~border], r32[~border].astype(np.float64))


@functools.lru_cache(maxsize=None)
def isotropic_reference(open_cap):
    v, f = sphere_case(open_cap)
    log = []
    out = isotropic_yardstick(v, f, 0.2 if open_cap else 0.12, 3, log=log)
    return out, log


def check_isotropic(dev, open_cap, dtype=torch.int64):
    """three iterations on the jittered icosphere.  The restatement's figures (printed, and in profiles/remesh_probe.md): closed, t = 0.12: share of
    edges below 4/5 t 0.160 -> 0.007 (bound 0.05), minimum edge 0.029 -> 0.091, valence-6 share 0.93, Euler characteristic 2 throughout; open,
    t = 0.2: Euler characteristic 1 throughout, all 28 open edges kept bit for bit."""
    v, f = sphere_case(open_cap)
    t = 0.2 if open_cap else 0.12
    (yv, yf, yp), log = isotropic_reference(open_cap)
    fin_, fy = figures(v, f, t), figures(yv, yf, t)
    print(f'isotropic open={open_cap} t={t}: input {fin_}')
    print(f'  restatement {fy}; per iteration (vertices, faces, collapses per round, flips per round): {log}')
    tv, tf, _ = _t(dev, v, f, dtype)
    builds = RT.BUILDS
    gv, gf, gp = MR.isotropic_remesh(tv, tf, t, 3)
    assert RT.BUILDS == builds + 1 and gf.dtype == dtype and gp.dtype == torch.int64                                  # one BVH of the input per call
    gv, gf, gp = gv.cpu().numpy(), gf.cpu().numpy().astype(np.int64), gp.cpu().numpy()
    fg = figures(gv, gf, t)
    print(f'  code under test {fg}')
    for name, (ov, of, op), fig in (('restatement', (yv, yf, yp), fy), ('code under test', (gv, gf, gp), fg)):
        check_invariants(v, f, ov, of, op, closed=not open_cap)
        assert fig['long'] <= fin_['long'] + 0.02, name
        if not open_cap:
            assert fig['short'] <= 0.05 and fig['min_edge'] > fin_['min_edge'], (name, fig)                           # the issue's figures for t = 0.12
        used = ov[np.unique(of)]                                                                                    # (the removed cap's vertices stay, unreferenced)
        on = closest_points(used, v, f)[0]
        assert np.abs(on - used.astype(np.float64)).max() <= 1e-6, name                                               # every vertex lies on the INPUT surface (float32 of a point on it)
    if open_cap:
        assert (HC._edges(gf)[1] == 1).sum() == (HC._edges(f)[1] == 1).sum() > 0                                     # every open edge is kept
    # without reprojection and with a pin mask the chain has no BVH in it: the restatement's smoothing is float32 with correctly rounded sqrt and
    # division, as the kernel's, so this comparison is exact
    pin = np.random.default_rng(9).random(len(v)) < 0.1
    yv, yf, yp = isotropic_yardstick(v, f, t, 1, pin=pin, reproject=False)
    tv, tf, tp = _t(dev, v, f, dtype, pin)
    builds = RT.BUILDS
    gv, gf, gp = MR.isotropic_remesh(tv, tf, t, 1, reproject=False, pin_mask=tp)
    assert RT.BUILDS == builds
    assert np.array_equal(gf.cpu().numpy(), yf) and np.array_equal(gp.cpu().numpy(), yp) and np.array_equal(_bits(gv.cpu().numpy()), _bits(yv))


def check_rejects(dev):
    """wrong shapes, dtypes, lengths and indices raise before any native call"""
    v, f = octahedron()
    tv, tf, _ = _t(dev, v, f)
    calls = []
    real = MR.L.call
    MR.L.call = lambda *a: calls.append(a)
    try:
        bad_v = (tv.double(), tv[:, :2], tv.reshape(-1))
        bad_f = (tf.float(), tf[:, :2], tf.reshape(-1), tf.to(torch.int16))
        bad_pin = (torch.zeros(len(v) + 1, dtype=torch.bool, device=dev), torch.zeros(len(v), dtype=torch.float32, device=dev))
        out_of_range = (tf.clone().index_put_((torch.tensor(0), torch.tensor(0)), torch.tensor(len(v))), tf.clone().index_put_((torch.tensor(1), torch.tensor(2)), torch.tensor(-1)))
        fns = (lambda v_, f_, p_=None: MR.collapse_short_edges(v_, f_, 0.1, 0.2, pin_mask=p_), lambda v_, f_, p_=None: MR.flip_edges(v_, f_, pin_mask=p_),
               lambda v_, f_, p_=None: MR.smooth_tangential(v_, f_, pin_mask=p_), lambda v_, f_, p_=None: MR.isotropic_remesh(v_, f_, 0.1, pin_mask=p_))
        for fn in fns:
            for x in bad_v:
                with pytest.raises(RuntimeError, match='positions'):
                    fn(x, tf)
            for x in bad_f:
                with pytest.raises(RuntimeError, match='faces'):
                    fn(tv, x)
            for x in bad_pin:
                with pytest.raises(RuntimeError, match='pin_mask'):
                    fn(tv, tf, x)
            for x in out_of_range:
                with pytest.raises(RuntimeError, match='outside'):
                    fn(tv, x)
        for bad in (0.0, -1.0, float('nan')):
            with pytest.raises(RuntimeError, match='target_len'):
                MR.isotropic_remesh(tv, tf, bad)
            with pytest.raises(RuntimeError, match='lo must'):
                MR.collapse_short_edges(tv, tf, bad, 1.0)
            with pytest.raises(RuntimeError, match='hi must'):
                MR.collapse_short_edges(tv, tf, 1.0, bad)
    finally:
        MR.L.call = real
    assert not calls


def check_wiring(dev, tmp_path):
    """remesh='split' (the default) writes the same bytes as before and builds no BVH; remesh='isotropic' gives files the seq stage's loader takes"""
    import script.process_body_cloth_head_msdfcut as PB
    from script.connet_face_head import om_loadmesh
    src = tmp_path / 'in'
    src.mkdir()
    paths = HC.write_scenario(src)
    kw = dict(wt_res=32, target_len=0.05, head_threshold=0.02)
    roots = {k: tmp_path / k for k in ('split', 'isotropic')}
    builds = RT.BUILDS
    PB.process_body_msdf_distance_bodyedge(None, str(roots['split']), *paths, **kw)                                 # the default
    assert RT.BUILDS == builds
    s = np.load(roots['split'] / 'merge_body_cloth.npz')
    s0 = int((s['face_labels'] == 0).sum())
    nb = int(s['f'][:s0].max()) + 1
    gv, gf = om_loadmesh(paths[1])
    rv, rf, _ = HC._refine(dev, gv, gf.astype(np.int64), 4.0 / 3.0 * 0.05, 3)                                        # today's route: the split alone, bit for bit
    assert np.array_equal(s['f'][s0:].astype(np.int64) - nb, rf) and np.array_equal(s['v'][nb:], rv.astype(np.float64))
    PB.process_body_msdf_distance_bodyedge(None, str(roots['isotropic']), *paths, remesh='isotropic', **kw)
    assert RT.BUILDS > builds
    with pytest.raises(RuntimeError, match='remesh'):
        PB.process_body_msdf_distance_bodyedge(None, str(tmp_path / 'bad'), *paths, remesh='meshlab', **kw)
    a = np.load(roots['isotropic'] / 'merge_body_cloth.npz')
    v, f, lab = a['v'], a['f'], a['face_labels']
    assert len(lab) == len(f) and f.min() >= 0 and f.max() < len(v)
    n0 = int((lab == 0).sum())
    assert np.all(lab[:n0] == 0) and np.all(lab[n0:] == 1) and 0 < n0 < len(lab)
    assert np.all(HC._edges(s['f'][:s0].astype(np.int64))[1] == 2) and np.all(HC._edges(f[:n0].astype(np.int64))[1] == 2)      # closed where 'split' is
    assert (HC._edges(f[n0:].astype(np.int64))[1] == 1).sum() == (HC._edges(s['f'][s0:].astype(np.int64))[1] == 1).sum()      # the garment's loops stay
    assert not np.array_equal(f, s['f'])
    from dataset.dataset_split import Dataset_split, DirectorySource, MemorySource, SMPLX_KEYS, _SMPLX_WIDTH

    class FromDirectory(MemorySource):
        def detail(self, process_path):
            return DirectorySource.detail(self, process_path)
    img, msk = np.zeros((8, 8, 3), np.uint8), np.zeros((8, 8), np.uint8)
    smplx = {k: np.zeros((2, _SMPLX_WIDTH[k]), np.float32) for k in SMPLX_KEYS}
    smplx.update(face_offset=np.zeros((1, 8, 3), np.float32), joint_offset=np.zeros((1, 55, 3), np.float32), locator_offset=np.zeros((1, 55, 3), np.float32),
                 shape_param=np.zeros((1, 100), np.float32))
    cam = {'intrinsic': np.array([[100.0, 0, 4], [0, 100.0, 4], [0, 0, 1]]), 'extrinsic': np.eye(4), 'height': 8, 'width': 8}
    ds = Dataset_split(FromDirectory([(img, msk, msk, msk, img)] * 2, (0, 1), smplx, cam), types.SimpleNamespace(device=dev, train_res=[8, 8]), Detail=True,
                       process_path=str(roots['isotropic']))
    assert ds.v.shape == (len(v), 3) and ds.f.shape == f.shape
