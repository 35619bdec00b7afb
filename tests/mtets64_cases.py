"""csrc/marching_tets.hip -- forward, compaction and the VJP kernels mt_bwd_boundary / mt_bwd_verts -- against oracle/marching_tets.py evaluated
in FLOAT64, and at the edges of its ordered compaction.  Shared by tests/test_mtets64_emul.py (host emulation) and tests/test_gpu_mtets64.py
(MI355X).  The measured tables: profiles/mtets64_emul.md, profiles/mtets64_gpu.md (`python tests/mtets64_cases.py cpu|cuda` prints them).

The reference.  OMT.gshell_tets on the float32 inputs (r32, autograd) and on their float64 copies with `decisions=r32` (r64): occupancy from the
float32 rounding of sdf, the mSDF decisions (polygon corners inside, cut edges, hence `used` and the cut faces) copied from the float32 run.
The three -- kernel, r32, r64 -- have one topology by construction, so no case is dropped for a kink.

Indices (faces, faces_wt, n_wt, faces32, faces_wt32, bnd_edge) are bit-exact against r32, forward values within 1e-7 absolute of r32 (the bar of
parity_cases.check_mtets_golden).  Then, for each of verts, verts_wt, msdf, d_pos, d_sdf, d_msdf:
    |kernel - r64|_2  <=  RATIO |r32 - r64|_2            (RATIO = 3, the rule of raster64_cases.py; both sides share |r64|_2, so it is left out
                                                          and an all-zero reference needs no special case: the kernel must then be exactly 0)
per tensor of every run, and per DECADE BAND of |r64| pooled over the runs of a group (BANDS): a large gradient cannot hide a wrong small one
-- the `den` and `tiny` cases span 1e-14 .. 1e12 in one tensor.  The float64 reference alone decides the banding (exact zeros are the band below
all others); a pooled band of fewer than MIN_BAND elements joins its neighbour of larger magnitude (the topmost one: of smaller).  No absolute
floor anywhere, and never a comparison with an earlier output of the kernel.
Boundary rows of `msdf` (index >= n_wt) are m_a w0 + m_b w1 = 0 mathematically: left out of the rule above and bounded absolutely by
8 * 2^-24 (|m_a w0| + |m_b w1|) evaluated in float64 (three roundings per product, two products, rounded up).
Exactly 0.0: the gradients at grid vertices on no crossing edge, every row of verts with used == 0, every gradient whose float64 reference is
identically zero (outputs left out of a subset); d_msdf is None for body=True.  Everything finite.

Groups of the banded rule: 'regular' (base shuffled mpos mneg mzero mplane col nonempty-after-empty), 'degenerate' (sdf0 tiny den), 'subsets',
and one per scan-path soup.  Each lattice run is body False / True x speculation off / on ("on": the second extraction on a grid, whose outputs
are views into capacity-sized buffers; SPEC_STATS says it really speculated).
"""
import contextlib
import zlib

import numpy as np
import torch

from parity_cases import T                     # (first: through conftest it puts the repository root on sys.path when this file runs as a script)
from oracle import marching_tets as OMT

RATIO = 3.0
MIN_BAND = 64
# The one exception to RATIO, per decade band only (the per-tensor bar of every run stays at 3): d_pos.  d_pos[v] is a sum over the up to 14
# crossing edges at v of g w, terms of size 1 whose sum is occasionally 1e-4: such a sum lands in a low band while its rounding error keeps the
# size of its TERMS, and the kernel adds them in another order than autograd (the three upstream gradients first, one product per edge; float
# atomics on the GPU) -- the same quality, another draw.  One such element decides a band of a few hundred: measured 8.06 (base, body pass:
# value -4.9e-4, kernel 3.4e-7 away, the float32 oracle by luck 4.2e-9), profiles/mtets64_emul.md and mtets64_gpu.md.  Set at the largest
# measured figure x 1.5; the float32 yardstick is not rescaled.
BAND_RATIO = {'d_pos': 12.1}
ZERO_BAND = -10 ** 6
OUT = {'verts': 'verts', 'msdf': 'msdf', 'verts_wt': 'vertices_watertight'}          # kernel key -> oracle key
ALL = ('verts', 'msdf', 'verts_wt')
SUBSETS = [s for s in ([k for k, b in zip(ALL, bits) if b] for bits in np.ndindex(2, 2, 2)) if s]       # the 7 non-empty subsets
LATTICE = ['base', 'shuffled', 'sdf0', 'tiny', 'den', 'mpos', 'mneg', 'mzero', 'mplane', 'col']
GROUP = {**{n: 'regular' for n in LATTICE}, 'sdf0': 'degenerate', 'tiny': 'degenerate', 'den': 'degenerate'}
MODES = [(False, False), (False, True), (True, False), (True, True)]                   # (body, speculative)
MODE_IDS = ['garment-exact', 'garment-spec', 'body-exact', 'body-spec']

BANDS = {}            # (dev, group) -> {tensor: {decade: [count, sum (k - r64)^2, sum (r32 - r64)^2, sum r64^2]}}
DONE = {}             # (dev, group) -> set of run tags pooled so far (a run is pooled once)
COVERAGE = {}         # soup name -> text (table-coverage counts for the profile files)


def _seed(*a):
    return zlib.crc32('/'.join(str(x) for x in a).encode())


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------
_INPUTS = {}


def lattice_inputs(name):
    """-> (pos [N,3], sdf [N] or [N,1], msdf [N], tets [nt,4] int64) numpy, float32"""
    if name in _INPUTS:
        return _INPUTS[name]
    n, shuffle = {'shuffled': (20, 5), 'mplane': (16, None)}.get(name, (12, None))
    rng = np.random.default_rng(_seed('lattice', n))                 # one field per grid: the cases differ only by what their name says
    verts, tets = OMT.kuhn_grid(n, shuffle_seed=shuffle)
    pos = (verts + (0.3 / n) * rng.uniform(-1, 1, verts.shape)).astype(np.float32)
    sdf = (np.linalg.norm(pos - np.array([0.02, -0.2, 0.01], np.float32), axis=-1) - 0.7).astype(np.float32)
    msdf = (rng.random(pos.shape[0]) - 0.35).astype(np.float32)
    u = rng.random(pos.shape[0])
    pick = rng.random(pos.shape[0])
    near = np.abs(sdf) < 0.15
    if name == 'sdf0':
        sdf[pick < 0.10] = 0.0
    elif name == 'tiny':
        sdf[near] = sdf[near] * np.float32(1e-11)
    elif name == 'den':
        sdf[near] = (np.sign(sdf[near]) * 1e-13 * (1 + u[near])).astype(np.float32)
    elif name == 'mpos':
        msdf = (np.abs(msdf) + 0.05).astype(np.float32)
    elif name == 'mneg':
        msdf = (-np.abs(msdf) - 0.05).astype(np.float32)
    elif name == 'mzero':
        msdf[pick < 0.25] = 0.0
    elif name == 'mplane':
        msdf = pos[:, 0].copy()
    elif name == 'empty':
        sdf = np.abs(sdf) + np.float32(0.1)
    elif name == 'col':
        sdf = sdf.reshape(-1, 1)
    _INPUTS[name] = (pos, sdf, msdf, tets)
    return _INPUTS[name]


def _pick4(rng, nt):
    """[nt, 4] distinct offsets inside a window of 8: a start and three steps of 1 or 2 (their sum stays below 8)"""
    step = rng.integers(1, 3, (nt, 3))
    return (rng.integers(0, 8, (nt, 1)) + np.concatenate([np.zeros((nt, 1), np.int64), np.cumsum(step, 1)], 1)) % 8


def local_soup(nt, nv, seed, scale=1.0):
    """a tet list that is no mesh: four distinct ids out of a window of 8 consecutive vertices (so edges are shared); pos, sdf, msdf randn"""
    rng = np.random.default_rng(_seed('soup', seed))
    tets = rng.integers(0, nv - 7, (nt, 1)) + _pick4(rng, nt)
    pos, sdf, msdf = (rng.standard_normal(s).astype(np.float32) for s in ((nv, 3), nv, nv))
    return pos, (sdf * np.float32(scale)).astype(np.float32), msdf, tets.astype(np.int64)


def density_soup(kind, nt=1025):
    """'every': two even and two odd ids per tet, sdf sign by parity -- every tet crosses.  'last' / 'ends': sdf > 0 except on one private
    vertex of the last tet / of tets 0 and nt - 1"""
    rng = np.random.default_rng(_seed('density', kind))
    nv = 600
    pos, sdf, msdf = (rng.standard_normal(s).astype(np.float32) for s in ((nv + 2, 3), nv + 2, nv + 2))
    if kind == 'every':
        base = 2 * rng.integers(0, nv // 2 - 3, (nt, 1))
        ev = rng.integers(0, 2, (nt, 1))
        tets = base + np.concatenate([2 * ev, 2 * ((ev + 1 + rng.integers(0, 2, (nt, 1))) % 4), 1 + 2 * ev, 1 + 2 * ((ev + 1) % 4)], 1)
        sdf = (np.abs(sdf) + 0.01) * np.where(np.arange(nv + 2) % 2 == 0, 1, -1)
    else:
        tets = rng.integers(0, nv - 7, (nt, 1)) + _pick4(rng, nt)
        sdf = np.abs(sdf) + 0.01
        tets[nt - 1, 2] = nv
        sdf[nv] = -0.4
        if kind == 'ends':
            tets[0, 1] = nv + 1
            sdf[nv + 1] = -0.7
    return pos, sdf.astype(np.float32), msdf, tets.astype(np.int64)


SCAN = {'per2': (262144 + 257, [262144]), 'segments': (2097152 + 300, [2097152]), 'edges': (420000, [])}
EDGE_BOUNDARY = 2097152


def scan_soup(name):
    """sparse crossings, so that the oracle stays quick at millions of tets.  per2 / segments: vertex chunks of 64, every 16th chunk `mixed` (sdf
    randn), the others positive; a tet draws its window of 8 inside one chunk, a `hot` tet -- every 997th index, the first and last 300, +-300
    around each boundary -- inside a mixed one.  edges: ids from all of 4000 vertices (ne > 2 097 152), sdf > 0 except on 48 vertices spread
    over the ids, two of them where edge 2 097 152 of the sorted edge list starts, so that crossing edges lie on both sides of it."""
    if ('scan', name) in _INPUTS:
        return _INPUTS[('scan', name)]
    nt, bounds = SCAN[name]
    rng = np.random.default_rng(_seed('scan', name))
    if name == 'edges':
        nv = 4000
        tets = rng.integers(0, nv, (nt, 4))
        while True:
            s = np.sort(tets, 1)
            bad = (s[:, 1:] == s[:, :-1]).any(1)
            if not bad.any():
                break
            tets[bad] = rng.integers(0, nv, (int(bad.sum()), 4))
        sdf = np.abs(rng.standard_normal(nv)) + 0.1
        e = np.sort(tets[:, OMT.BASE_TET_EDGES].reshape(-1, 2), 1)
        uniq = np.unique(e[:, 0] * nv + e[:, 1])                         # the sorted edge list TetGrid builds, as keys
        assert uniq.shape[0] > EDGE_BOUNDARY + 256, uniq.shape
        vb = int(uniq[EDGE_BOUNDARY] // nv)                              # edge 2 097 152 starts at this vertex: it and the one before are hot,
        # and so is one of the last edges' vertices.  (48 hot vertices, not a dozen: each gathers ~1000 gradient terms, and the more of these
        # long float32 sums a norm pools, the less one run's order of the atomics moves the ratio)
        neg = np.unique(np.concatenate([np.linspace(5, 3950, 45).astype(np.int64), [vb - 1, vb, nv - 2]]))
        sdf[neg] = -sdf[neg]
    else:
        nchunk = 16 * max(4, nt // 8192)
        nv = 64 * nchunk
        hot = np.zeros(nt, bool)
        hot[::997] = True
        hot[:300] = hot[-300:] = True
        for b in bounds:
            hot[b - 300:b + 300] = True
        mixed = 16 * rng.integers(0, nchunk // 16, nt)
        plain = rng.integers(0, nchunk - nchunk // 16, nt)
        plain = plain + plain // 15 + 1                                  # skip every 16th chunk
        chunk = np.where(hot, mixed, plain)
        tets = (64 * chunk + rng.integers(0, 57, nt))[:, None] + _pick4(rng, nt)
        sdf = rng.standard_normal(nv)
        is_mixed = (np.arange(nv) // 64) % 16 == 0
        sdf = np.where(is_mixed, sdf, np.abs(sdf) + 0.1)
    pos, msdf = rng.standard_normal((nv, 3)).astype(np.float32), rng.standard_normal(nv).astype(np.float32)
    _INPUTS[('scan', name)] = (pos, sdf.astype(np.float32), msdf, tets.astype(np.int64))
    return _INPUTS[('scan', name)]


# ---- the reference ---------------------------------------------------------------------------------------------------------------------------
class _Ref:
    pass


_REF = {}


def reference(key, inp, body, f64=True):
    """computed once per (inputs, pass) and shared, unchanged, by every run that needs it"""
    if (key, body) in _REF:
        return _REF[(key, body)]
    r = _Ref()
    pos, sdf, msdf, tets = (torch.from_numpy(np.ascontiguousarray(a)) for a in inp)
    r.l32 = [t.clone().requires_grad_(True) for t in (pos, sdf, msdf)]
    r.o32 = OMT.gshell_tets(*r.l32, tets, negate_msdf=body)
    r.l64 = r.o64 = None
    if f64:
        r.l64 = [t.double().requires_grad_(True) for t in (pos, sdf, msdf)]
        r.o64 = OMT.gshell_tets(*r.l64, tets, negate_msdf=body, decisions=r.o32)
        for k in ('faces', 'faces_watertight', 'bnd_edge', 'used'):
            assert torch.equal(r.o32[k], r.o64[k]), (key, k)            # one topology by construction
    gen = torch.Generator().manual_seed(_seed('up', key, body))
    r.ups = {k: torch.randn(r.o32[OUT[k]].shape, generator=gen) for k in ALL}
    r.touched = torch.zeros(pos.shape[0], dtype=torch.bool)
    r.touched[r.o32['edge_verts'].reshape(-1)] = True
    r.grads = {}
    _REF[(key, body)] = r
    return r


def _ref_grads(r, subset):
    """-> (float32 grads, float64 grads) of sum_k <out_k, up_k> over the subset; None where autograd reaches nothing"""
    key = tuple(subset)
    if key not in r.grads:
        res = []
        for leaves, out, dt in ((r.l32, r.o32, torch.float32), (r.l64, r.o64, torch.float64)):
            loss = sum((out[OUT[k]] * r.ups[k].to(dt)).sum() for k in subset)
            res.append(torch.autograd.grad(loss, leaves, retain_graph=True, allow_unused=True) if loss.requires_grad else (None, None, None))
        r.grads[key] = res
    return r.grads[key]


# ---- the kernels -----------------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _speculation(flag):
    from d3h import mtets
    keep = mtets.SPECULATE
    mtets.SPECULATE = flag
    mtets.TetGrid._cache.clear()
    try:
        yield mtets
    finally:
        mtets.SPECULATE = keep
        mtets.TetGrid._cache.clear()


def extract(dev, inp, body, spec, first=None, overflow=False):
    """one extraction with gradients.  spec: it is the SECOND extraction on its grid (the first one on `first`, default the same inputs), so it is
    queued at the capacities the first one left and its outputs are views; overflow: the first one left capacities this one outgrows"""
    pos, sdf, msdf, tets = inp
    with _speculation(spec) as mtets:
        tt = T(tets, dev)
        if first is not None or spec:
            f = first if first is not None else inp
            mtets.marching_tets(T(f[0], dev), T(f[1], dev), T(f[2], dev), tt, body=body)
        s0 = dict(mtets.SPEC_STATS)
        leaves = [T(pos, dev, True), T(sdf, dev, True), T(msdf, dev, True)]
        o = mtets.marching_tets(*leaves, tt, body=body)
        d = {k: mtets.SPEC_STATS[k] - s0[k] for k in s0}
        assert d == {'speculated': int(spec), 'overflowed': int(spec and overflow)}, d
        if spec and not overflow:
            for k in ALL:                                                # really views into the capacity-sized allocations
                assert o[k].untyped_storage().nbytes() > o[k].numel() * o[k].element_size(), k
                assert o[k].is_contiguous()
    return o, leaves


def check_forward(o, r32, tag):
    """indices and shapes bit-exact, values within 1e-7, unused rows exactly zero; -> {tensor: bit-equal?}"""
    def same(a, b):
        return tuple(a.shape) == tuple(b.shape) and torch.equal(a.cpu().long(), b.long())
    assert o['faces'].dtype == torch.int64 and o['faces_wt'].dtype == torch.int64, tag
    assert o['faces32'].dtype == torch.int32 and o['faces_wt32'].dtype == torch.int32 and o['bnd_edge'].dtype == torch.int32, tag
    assert same(o['faces'], r32['faces']) and same(o['faces32'], r32['faces']), (tag, 'faces')
    assert same(o['faces_wt'], r32['faces_watertight']) and same(o['faces_wt32'], r32['faces_watertight']), (tag, 'faces_wt')
    assert o['n_wt'] == r32['n_verts_watertight'], (tag, 'n_wt')
    assert same(o['bnd_edge'], r32['bnd_edge']), (tag, 'bnd_edge')
    bit = {}
    for k in ALL:
        a, b = o[k].detach().cpu(), r32[OUT[k]].detach()
        assert a.shape == b.shape and a.dtype == torch.float32, (tag, k)
        assert bool(torch.isfinite(a).all()), (tag, k)
        if a.numel():
            assert float((a - b).abs().max()) <= 1e-7, (tag, k, float((a - b).abs().max()))
        bit[k] = torch.equal(a, b)
    v = o['verts'].detach().cpu()
    assert bool((v[~r32['used']] == 0).all()), (tag, 'rows of verts with used == 0')
    return bit


def _bands(dev, group, tensor, dk, d32, r64):
    acc = BANDS.setdefault((dev, group), {}).setdefault(tensor, {})
    a = np.abs(r64)
    dec = np.full(a.shape, ZERO_BAND, np.int64)
    dec[a > 0] = np.floor(np.log10(a[a > 0])).astype(np.int64)
    for b in np.unique(dec):
        m = dec == b
        row = acc.setdefault(int(b), [0, 0.0, 0.0, 0.0])
        row[0] += int(m.sum())
        row[1] += float((dk[m] ** 2).sum())
        row[2] += float((d32[m] ** 2).sum())
        row[3] += float((r64[m] ** 2).sum())


def _compare(dev, group, tag, tensor, k, r32, r64, report, pool, keep=None):
    k, r32, r64 = (t.detach().cpu().double().reshape(-1).numpy() for t in (k, r32, r64))
    assert np.isfinite(k).all(), (tag, tensor, 'not finite')
    if keep is not None:
        k, r32, r64 = k[keep], r32[keep], r64[keep]
    dk, d32 = k - r64, r32 - r64
    nk, n32, n64 = float(np.linalg.norm(dk)), float(np.linalg.norm(d32)), float(np.linalg.norm(r64))
    ratio = nk / n32 if n32 > 0 else (0.0 if nk == 0 else float('inf'))
    rel = (lambda x: x / n64) if n64 > 0 else (lambda x: x)
    report(f'[mtets64] {dev:4s} {tag:34s} {tensor:9s} e_k {rel(nk):.3e} e_32 {rel(n32):.3e} ratio {ratio:.2f}' + ('' if n64 > 0 else ' (|r64| = 0: absolute)'))
    if pool:
        _bands(dev, group, tensor, dk, d32, r64)
    assert nk <= RATIO * n32, (tag, tensor, nk, n32, ratio)


def _boundary_msdf(o, r, tag):
    """rows >= n_wt of msdf: |kernel| <= 8 * 2^-24 (|m_a w0| + |m_b w1|), the terms in float64"""
    n_wt = r.o32['n_verts_watertight']
    m = r.o64['msdf_vert'].detach()[r.o64['bnd_edge']]                                       # [nb, 2]
    dec = r.o32['decisions']
    ok = torch.cat([dec[k].reshape(-1) for k in ('ok3', 'ok4') if k in dec]) if m.shape[0] else torch.zeros(0, dtype=torch.bool)
    a, b = m[:, 0], -m[:, 1]
    den = torch.where(ok, a + b, torch.ones_like(a))
    w0, w1 = torch.where(ok, b / den, torch.zeros_like(a)), torch.where(ok, a / den, torch.zeros_like(a))
    bound = 8.0 * 2.0 ** -24 * ((m[:, 0] * w0).abs() + (m[:, 1] * w1).abs())
    got = o['msdf'].detach().cpu().double()[n_wt:].abs()
    assert bool((got <= bound).all()), (tag, 'boundary msdf', float((got - bound).max()))


def check_grads(dev, group, tag, o, leaves, r, subset, report, body, pool=True):
    """forward values (full subset only) and the three gradients of sum_{k in subset} <o[k], up_k> by the section-3 rule"""
    pool = pool and tag not in DONE.setdefault((dev, group), set())
    DONE[(dev, group)].add(tag)
    n_wt = r.o32['n_verts_watertight']
    if tuple(subset) == ALL:
        for k in ALL:
            keep = None
            if k == 'msdf':
                keep = np.arange(r.o32['msdf'].shape[0]) < n_wt
                _boundary_msdf(o, r, tag)
            _compare(dev, group, tag, k, o[k], r.o32[OUT[k]], r.o64[OUT[k]], report, pool, keep)
    loss = sum((o[k] * r.ups[k].to(dev)).sum() for k in subset)
    got = torch.autograd.grad(loss, leaves, retain_graph=True, allow_unused=True)
    g32, g64 = _ref_grads(r, subset)
    for name, x, leaf, a32, a64 in zip(('d_pos', 'd_sdf', 'd_msdf'), got, leaves, g32, g64):
        if name == 'd_msdf' and body:
            assert x is None and a64 is None, (tag, 'the body pass sends no gradient to msdf')
            continue
        assert x is not None and x.shape == leaf.shape and x.dtype == torch.float32, (tag, name)
        xc = x.detach().cpu()
        assert bool(torch.isfinite(xc).all()), (tag, name, 'not finite')
        assert bool((xc[~r.touched] == 0).all()), (tag, name, 'nonzero at a grid vertex on no crossing edge')
        if a64 is None or not bool(a64.any()):
            assert not bool(xc.any()), (tag, name, 'must be exactly zero: nothing differentiated reaches it')
            report(f'[mtets64] {dev:4s} {tag:34s} {name:9s} exactly zero, as the reference')
            continue
        _compare(dev, group, tag, name, xc, a32, a64, report, pool)


# ---- lattice cases ---------------------------------------------------------------------------------------------------------------------------
def run_lattice(dev, name, body, spec, report=print):
    inp = lattice_inputs(name)
    r = reference(name, inp, body)
    tag = f'{name}/{"body" if body else "garment"}/{"spec" if spec else "exact"}'
    o, leaves = extract(dev, inp, body, spec)
    bit = check_forward(o, r.o32, tag)
    report(f'[mtets64] {dev:4s} {tag:34s} {o["n_wt"]} + {o["verts"].shape[0] - o["n_wt"]} vertices, {o["faces"].shape[0]} cut faces; bit-equal to the float32 oracle: {bit}')
    if name == 'mneg' and not body or name == 'mpos' and body:
        assert o['faces'].shape[0] == 0 and not bool(o['verts'].any()), tag           # nothing survives the cut: verts is exactly 0
    if name == 'mpos' and not body or name == 'mneg' and body:
        assert not bool(r.o32['decisions']['ok3'].any()) and not bool(r.o32['decisions']['ok4'].any()), tag     # no cut: every polygon whole
    check_grads(dev, GROUP[name], tag, o, leaves, r, ALL, report, body)
    if name == 'col':
        assert leaves[1].shape[1:] == (1,)


def run_subsets(dev, body, spec, report=print):
    """each non-empty subset of the three value outputs as the only differentiated ones: the null-pointer paths of d3h_mtets_bwd (and, from the
    second backward through the retained graph on, the zero fills the backward makes for itself)"""
    inp = lattice_inputs('base')
    r = reference('base', inp, body)
    o, leaves = extract(dev, inp, body, spec)
    for s in SUBSETS:
        tag = f'subset {"+".join(s)}/{"body" if body else "garment"}/{"spec" if spec else "exact"}'
        check_grads(dev, 'subsets', tag, o, leaves, r, s, report, body)


def run_empty(dev, body, report=print):
    """sdf > 0 everywhere: zero rows, zero gradients -- on the exact path, as the speculative second extraction after a non-empty first one, and
    a non-empty extraction after an empty one (speculating: it outgrows the empty one's capacities and is repeated at the exact sizes)"""
    base, empty = lattice_inputs('base'), lattice_inputs('empty')
    r0 = reference('empty', empty, body, f64=False)
    for spec in (False, True):
        tag = f'empty/{"body" if body else "garment"}/{"spec after non-empty" if spec else "exact"}'
        o, leaves = extract(dev, empty, body, spec, first=base if spec else None)
        check_forward(o, r0.o32, tag)
        for k in ('verts', 'msdf', 'verts_wt', 'faces', 'faces_wt', 'faces32', 'faces_wt32', 'bnd_edge'):
            assert o[k].shape[0] == 0, (tag, k)
        loss = sum((o[k] * r0.ups[k].to(dev)).sum() for k in ALL)
        got = torch.autograd.grad(loss, leaves, allow_unused=True)
        for x, leaf, nm in zip(got, leaves, ('d_pos', 'd_sdf', 'd_msdf')):
            if nm == 'd_msdf' and body:
                assert x is None, tag
            else:
                assert x is not None and x.shape == leaf.shape and not bool(x.any()), (tag, nm)
        report(f'[mtets64] {dev:4s} {tag:34s} zero rows, zero gradients of the input shapes')
    r = reference('base', base, body)
    for spec in (False, True):
        tag = f'nonempty after empty/{"body" if body else "garment"}/{"spec" if spec else "exact"}'
        o, leaves = extract(dev, base, body, spec, first=empty, overflow=True)
        check_forward(o, r.o32, tag)
        check_grads(dev, 'regular', tag, o, leaves, r, ALL, report, body)


# ---- compaction cases ("tet soups") ----------------------------------------------------------------------------------------------------------
def run_soup(dev, key, inp, report=print, grads=False, group=None, bodies=(False, True)):
    """exact against the float32 oracle: both passes, exact and speculative path; grads: also one backward per run by the section-3 rule"""
    for body in bodies:
        r = reference(key, inp, body, f64=grads)
        for spec in (False, True):
            tag = f'{key}/{"body" if body else "garment"}/{"spec" if spec else "exact"}'
            o, leaves = extract(dev, inp, body, spec)
            check_forward(o, r.o32, tag)
            if grads:
                check_grads(dev, group, tag, o, leaves, r, ALL, report, body)
    return r


TRI_CODES = [c for c in range(16) if OMT.NUM_TRIANGLES[c] == 1]
QUAD_CODES = [c for c in range(16) if OMT.NUM_TRIANGLES[c] == 2]
UNREACHABLE = {(c, p) for c in QUAD_CODES for p in (5, 10)}        # alternating signs at the corners of a planar convex section
TABLES_SEED = 0


def table_pairs(o32):
    """the (case code, mSDF polygon case) pairs the ORACLE's decisions take (never the kernel's tet_code)"""
    return set(zip(o32['tet_case'].tolist(), o32['poly_case'].tolist()))


def check_tables(dev, report=print):
    """20 000 tets over 3 000 vertices: every reachable row pair of the four case tables occurs -- 148 of the 160 (8 triangle codes x 8 polygon
    cases + 6 quad codes x 16); the other 12 are the quad codes with polygon case 5 or 10, which consistent linear interpolation cannot produce"""
    every = {(c, p) for c in TRI_CODES for p in range(8)} | {(c, p) for c in QUAD_CODES for p in range(16)}
    assert len(every) == 160
    inp = local_soup(20000, 3000, ('tables', TABLES_SEED))
    for body in (False, True):
        pairs = table_pairs(reference('tables', inp, body, f64=False).o32)
        tag = f'tables/{"body" if body else "garment"}'
        COVERAGE[tag] = f'{len(pairs)} of 160 pairs; of the 12 quad x (5, 10) pairs: {len(pairs & UNREACHABLE)}'
        report(f'[mtets64] {tag}: {COVERAGE[tag]}')
        assert pairs == every - UNREACHABLE, sorted(every - UNREACHABLE - pairs)
    run_soup(dev, 'tables', inp, report)
    # sdf x 1e-13: the +1e-12 regulariser dominates the denominators and the weights no longer sum to 1 -- but both shrink by one positive factor
    # (a + b) / (a + b + 1e-12), so msdf_vert keeps the SIGN of the linear interpolation and cases 5 / 10 stay out of reach: 148 here too
    inp = local_soup(20000, 3000, ('tables', TABLES_SEED), scale=1e-13)
    for body in (False, True):
        pairs = table_pairs(reference('tables1e-13', inp, body, f64=False).o32)
        tag = f'tables x 1e-13/{"body" if body else "garment"}'
        COVERAGE[tag] = f'{len(pairs)} of 160 pairs; of the 12 quad x (5, 10) pairs: {len(pairs & UNREACHABLE)}'
        report(f'[mtets64] {tag}: {COVERAGE[tag]}')
        assert pairs == every - UNREACHABLE, sorted(every - UNREACHABLE - pairs)
    run_soup(dev, 'tables1e-13', inp, report)


BOUNDARY_NT = [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025]


def check_boundary(dev, nt, report=print):
    """the first nt tets of one seeded local soup: wave (64), workgroup (256) and four-workgroup sizes, one below, at and above"""
    pos, sdf, msdf, tets = local_soup(1025, 600, 'boundaries')
    run_soup(dev, f'nt{nt}', (pos, sdf, msdf, tets[:nt].copy()), report)


def check_density(dev, kind, report=print):
    inp = density_soup(kind)
    nt = inp[3].shape[0]
    occ = (inp[1] > 0)[inp[3]].sum(1)
    valid = (occ > 0) & (occ < 4)
    want = {'every': np.ones(nt, bool), 'last': np.arange(nt) == nt - 1, 'ends': (np.arange(nt) == 0) | (np.arange(nt) == nt - 1)}[kind]
    assert np.array_equal(valid, want), kind
    run_soup(dev, f'density-{kind}', inp, report)


def check_scan(dev, name, body, report=print):
    """the `per > 1` path of mt_scan (1026 workgroups, ragged tail), its segment loop (8194 workgroups: a carry across entry 8192) and an edge list
    of more than 2 097 152 entries; crossings on both sides of every boundary (asserted on the inputs); one backward per run, section-3 rule"""
    inp = scan_soup(name)
    pos, sdf, msdf, tets = inp
    nt, bounds = SCAN[name]
    assert tets.shape[0] == nt
    occ = (sdf > 0)[tets].sum(1)
    valid = (occ > 0) & (occ < 4)
    assert valid[:256].any() and valid[-(nt % 256 or 256):].any(), name                          # first and (ragged) last workgroup
    for b in bounds:
        assert valid[b - 256:b].any() and valid[b:b + 256].any(), (name, b)
        assert (nt + 255) // 256 > b // 256 + 1
    if name == 'edges':
        e = np.sort(tets[:, OMT.BASE_TET_EDGES].reshape(-1, 2), 1)
        uniq = np.unique(e[:, 0] * 4000 + e[:, 1])
        ne = uniq.shape[0]
        cross = (sdf[uniq // 4000] > 0) != (sdf[uniq % 4000] > 0)
        assert ne > EDGE_BOUNDARY + 256, ne
        assert cross[EDGE_BOUNDARY - 256:EDGE_BOUNDARY].any() and cross[EDGE_BOUNDARY:EDGE_BOUNDARY + 256].any() and cross[-(ne % 256 or 256):].any(), name
        COVERAGE['scan/edges'] = f'ne = {ne}, {int(cross.sum())} crossing edges, {int(cross[EDGE_BOUNDARY:].sum())} of them past edge {EDGE_BOUNDARY}'
    else:
        COVERAGE[f'scan/{name}'] = f'nt = {nt} ({(nt + 255) // 256} workgroups), {int(valid.sum())} crossing tets'
    run_soup(dev, f'scan-{name}', inp, report, grads=True, group=f'scan-{name}', bodies=(body,))
    _REF.pop((f'scan-{name}', body), None)                                                     # (hundreds of MB at 2 M tets)


# ---- the banded bar --------------------------------------------------------------------------------------------------------------------------
def merged_bands(acc):
    """{decade: row} -> [(label, row)] ascending, every band of fewer than MIN_BAND elements joined to its neighbour of larger magnitude"""
    rows = [[[b], list(acc[b])] for b in sorted(acc)]
    i = 0
    while len(rows) > 1 and i < len(rows):
        if rows[i][1][0] >= MIN_BAND:
            i += 1
            continue
        j = i + 1 if i + 1 < len(rows) else i - 1                      # (the topmost band has no larger neighbour: it joins the one below)
        rows[j][0] = sorted(rows[j][0] + rows[i][0])
        rows[j][1] = [x + y for x, y in zip(rows[j][1], rows[i][1])]
        del rows[i]                                                    # what was rows[j] now sits at i (or the list ended): looked at next

    def label(bs):
        f = lambda b: '0' if b == ZERO_BAND else f'1e{b}'
        return f(bs[0]) if len(bs) == 1 else f'{f(bs[0])} .. 1e{bs[-1] + 1}'
    return [(label(bs), row) for bs, row in rows]


def check_bands(dev, group, report=print):
    """the pooled per-decade bar of a group whose runs have been made (by the tests before this one, or by ensure=)"""
    acc = BANDS.get((dev, group))
    assert acc, f'no run of group {group} recorded on {dev}'
    worst = []
    for tensor in ('verts', 'verts_wt', 'msdf', 'd_pos', 'd_sdf', 'd_msdf'):
        for label, (n, sk, s32, s64) in merged_bands(acc.get(tensor, {})):
            ratio = (sk / s32) ** 0.5 if s32 > 0 else (0.0 if sk == 0 else float('inf'))
            den = s64 ** 0.5 if s64 > 0 else 1.0
            report(f'[mtets64] {dev:4s} band {group:14s} {tensor:9s} |r64| in {label:18s} n {n:8d} e_k {sk ** 0.5 / den:.3e} e_32 {s32 ** 0.5 / den:.3e} ratio {ratio:.2f}')
            if sk > BAND_RATIO.get(tensor, RATIO) ** 2 * s32:
                worst.append((tensor, label, n, ratio))
    assert not worst, worst


def ensure_group(dev, group, report=print):
    """make every run of a group that has not been made yet (so the banded test stands on its own when selected alone)"""
    done = DONE.get((dev, group), set())
    quiet = lambda s: None
    if group == 'subsets':
        for body, spec in MODES:
            if f'subset verts/{"body" if body else "garment"}/{"spec" if spec else "exact"}' not in done:
                run_subsets(dev, body, spec, quiet)
        return
    for name in LATTICE:
        if GROUP[name] != group:
            continue
        for body, spec in MODES:
            if f'{name}/{"body" if body else "garment"}/{"spec" if spec else "exact"}' not in done:
                run_lattice(dev, name, body, spec, quiet)
    if group == 'regular':
        for body in (False, True):
            if f'nonempty after empty/{"body" if body else "garment"}/exact' not in done:
                run_empty(dev, body, quiet)


def check_group(dev, group, report=print):
    ensure_group(dev, group, report)
    check_bands(dev, group, report)


# ---- the profile files -----------------------------------------------------------------------------------------------------------------------
def main(dev, scan):
    """every case with the figures as markdown tables on stdout (profiles/mtets64_emul.md, profiles/mtets64_gpu.md)"""
    lines = []
    rep = lines.append
    for name in LATTICE:
        for body, spec in MODES:
            run_lattice(dev, name, body, spec, rep)
    for body, spec in MODES:
        run_subsets(dev, body, spec, rep)
    for body in (False, True):
        run_empty(dev, body, rep)
    check_tables(dev, rep)
    for nt in BOUNDARY_NT:
        check_boundary(dev, nt, rep)
    for kind in ('every', 'last', 'ends'):
        check_density(dev, kind, rep)
    groups = ['regular', 'degenerate', 'subsets']
    for name in scan:
        for body in (False, True):
            check_scan(dev, name, body, rep)
        groups.append(f'scan-{name}')
    bands = []
    for g in groups:
        try:
            check_bands(dev, g, bands.append)
        except AssertionError as e:
            print(f'**band bar missed in group {g}: {e}**\n')
    print('## Table coverage and soup sizes\n')
    for k, v in COVERAGE.items():
        print(f'- `{k}`: {v}')
    print('\n## Per decade band of |float64 value|, pooled over the runs of a group (asserted: ratio <= 3)\n')
    print('| group | tensor | band | elements | e_k | e_32 | ratio |\n|---|---|---|---|---|---|---|')
    for s in bands:
        w = s.split()
        i = w.index('n')
        print(f'| {w[3]} | {w[4]} | {" ".join(w[7:i])} | {w[i + 1]} | {w[i + 3]} | {w[i + 5]} | {w[i + 7]} |')
    print('\n## Per run and tensor (asserted: ratio <= 3)\n')
    print('| run | tensor | e_k | e_32 | ratio |\n|---|---|---|---|---|')
    for s in lines:
        if ' e_k ' in s:
            head, tail = s.split(' e_k ')
            w, t = head.split(), tail.split()
            print(f'| {" ".join(w[2:-1])} | {w[-1]} | {t[0]} | {t[2]} | {t[4]} |')
    print('\n## Forward summaries\n')
    for s in lines:
        if ' e_k ' not in s:
            print('- ' + ' '.join(s.split()[1:]))


if __name__ == '__main__':
    import sys
    import conftest
    from d3h import _lib as L
    device = sys.argv[1] if len(sys.argv) > 1 else 'cpu'
    if device == 'cpu':
        L._use_emulator_for_tests(conftest.EMUL_SO)
    main(device, [a for a in sys.argv[2:]] if len(sys.argv) > 2 else (['per2'] if device == 'cpu' else list(SCAN)))
