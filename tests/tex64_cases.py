"""The hash-grid texture of csrc/texmlp.hip -- the five-level encoding, the 10 -> 32 -> 32 -> 6 MLP, the table scatter and the position gradient
-- against FLOAT64, per element and at its edges.  Shared by tests/test_tex64_emul.py (host emulation) and tests/test_gpu_tex64.py (MI355X).
The measured tables: profiles/tex64_emul.md, profiles/tex64_gpu.md (`python tests/tex64_cases.py cpu|cuda` prints them).

The reference.  The op restated in torch with the dtype as a parameter (ref_eval): x_n = clamp((x - b0) / (b1 - b0), 0, 1) -- a division, as
in the kernel --, the encoding (p = x_n scale + 0.5, trilinear over the 8 corners of floor(p), dense index with the level's wrap), the x
in_grad_scale hook on the encoding's gradient, the bias-free ReLU MLP, sigmoid (omax - omin) + omin, masked pixels zero.  Evaluated on the
float32 inputs (r32) and on their float64 copies (r64); gradients by autograd in the same dtype.  The level scales are the float32 values of
oracle.texmlp.grid_layout() widened (what make_cfg computes); box and output ranges are float32 values widened.  Never a comparison with an
earlier output of the kernel, except rule (d).

Routes (each with value or gradient checks; `wrap` goes through d3h.texmlp, the numbered ones through L.call with poisoned buffers):
  1  texmlp_fwd, out only                     texmlp_fwd_mfma_kernel
  2  texmlp_fwd, enc_out only (unit box) and out + enc_out together          texmlp_fwd_kernel
  3  the default backward: MLP half with d_x (h2<true>), then the table scatter as its own enc_only call (<1>); `wrap`: the same through
     texture_mlp(...).backward(), on the GPU with the scatter on the side stream
  4  one call with d_table, d_w, d_x and the scratch (what ASYNC_TABLE_GRAD = False issues): h2<true>, then <1> with the table only
  5  the three calls d3h.texmlp issues with DX_FUSED off: h2<false>, then <1> with d_x, then <1> with the table
  5e one call with everything under D3H_TEX_DX_FUSED=0 (the switch inside d3h_texmlp_bwd): h2<false>, then <1> with d_x and the table
  6  x without grad: h2<false>, then <1> with the table
  7  texmlp_bwd with genc_scratch = NULL: texmlp_bwd_kernel<0>
  8  grid_encode backward: <1>, unit box, a 10-channel gradient
The grids: an enc_only call (route 8, and the scatter of routes 3, 5 and `wrap`) launches <1> on at most 1021 workgroups; the 4093-workgroup
launch of <1> is the second half of a ONE-call backward (routes 4, 5e, 6) and of nothing else -- the side-stream scatter of the default backward
is an enc_only call.  `loops bwd 1021` gives the 1021-wide launches (routes 3, 5, 7, 8, wrap) a second tile, `loops scatter 4093` the 4093-wide
one (routes 4, 5e, 6), each with a tile mask laid out for that width.
D3H_TEX_H2=0 and D3H_TEX_MERGE_FACES=0 are read once into statics and cannot be switched inside a process: both A/B relics are left out.

(a) Per-element tensors (out, the encoding, d_x, genc, d_table, the three weight gradients):
        |kernel - r64|_2  <=  RATIO |r32 - r64|_2,     RATIO = 3,
    per tensor of every run (tensors of >= MIN_BAND elements) and per DECADE BAND of |r64| pooled over the runs of a group (the joining rule
    of mtets64_cases.merged_bands).  No absolute floor: where r64 is exactly zero and r32 is, the kernel must be.  Exceptions by name in
    BAND_RATIO, for what passes through the h2 chain only, bar = measured x 1.5 and never above 8: 2^-21 relative per product is all a
    two-plane split of both operands can justify against 2^-24.  Tensors are named tensor/route, so a band is pooled per route.
(b) d_table and the weight gradients are sums; a band of near-cancelling sums could be held to L 2^-24 sum |term| instead, with L counted from
    the code (d_w: tiles per wave x 2 chains + 32 products of one MFMA contraction + 1 + 3 for the LDS reduction + one float atomic per workgroup;
    d_table: 6 steps of the segmented wave scan + 1 face fold + the contributions to the address).  No band needed it on either device: (a)
    holds in every band of every sum, so nothing of (b) is implemented.
(c) Exact results, on NaN-poisoned out / d_x / genc and on d_table / d_w pre-filled with -0.0 (x + (-0.0) == x bit for bit, and an entry no
    atomic touched still has its sign bit): `out` rows of masked pixels are 0 in all six channels; d_x rows of masked pixels are 0; d_x[d] is
    0 for a coordinate clamped on axis d; d_x is 0 where the pixel has no upstream gradient; no NaN is left in out or d_x for any n; table
    entries no covered pixel WITH an upstream gradient addresses and, where nothing contributes at all, every d_w are still -0.0; genc of a
    covered pixel without an upstream gradient is written, as 0 (`edges zero-gradient`: whole chains, first / second chain of a wave, a whole
    wave and single pixels without a gradient among live ones).
(d) Routes 3, 4, 5, 7 on the same inputs: each meets (a), and the d_x of 3 and 4 are bit-equal (same kernel, same data).

Mixed chains (one 32-pixel chain holds pixels at 1, 1e-2, 1e-4, 1e-6, 1e-8 of its largest gradient): the pixels down to 1e-4 are held to
(a) per level.  d_table of this case is held per tensor only, not per band: an entry fed by 1e-6 and 1e-8 pixels alone inherits their error,
which (a) does not bound; what bounds it is the per-pixel rule below on genc, of which the entry is a float32 sum.  At 1e-6 and 1e-8 the error belongs to the chain's largest.  With S the chain's power-of-two scale (largest |go| S in [32, 64))
every B operand of the backward chain is b_h + 2^-11 b_m', two fp16 planes; the low plane bottoms out at the fp16 subnormal step 2^-24, which
is d = 2^-35 in scaled units, so an operand is off by at most d + 2^-22 |b|.  Per pixel, through the three layers,
        |genc - r64| <= (gs / S) [ |W1^T| ( |W2^T| ( |W3^T| d 1_6 + d 1_32 ) + d 1_32 )  +  8 2^-24 |W1^T| |W2^T| |W3^T| |go S| ]
(ReLU derivatives bounded by 1; the second term is the 2^-21 relative allowance, (a)'s ceiling) and |d_x - r64| <= sum_c |d enc_c / d x|
times that.  Asserted; the largest fraction of the bound is recorded for both devices.  The bound needs the subnormals: a matrix pipe that
flushed fp16 subnormal operands to zero would lose the whole high plane of a 1e-6 pixel (|go S| < 2^-14), 10^5 times this bound.

Input hygiene (asserted on the inputs, not a tolerance): ReLU kinks and cell faces are discontinuities of the derivative.  Random points
are redrawn until, in float64, every hidden pre-activation has |z_i| >= KINK sum_j |w_ij h_j| (KINK = 2^-16) and every p = x_n scale + 0.5
is at least FACE = 1e-5 from an integer; at most 5 % of the points per round, at most 8 rounds, none left.  Cases with prescribed positions
(runs, curves, the shell) give offending pixels mask = 0 in kernel and reference alike, at most 2 % of a case.  Lattice-point cases (p an
integer on purpose) check the forward, which is continuous there, and that d_x is one of the two one-sided float64 derivatives (check_one_sided).
"""
import math
import os
import zlib

import numpy as np
import torch

from parity_cases import T                     # noqa: F401  (first: through conftest it puts the repository root on sys.path when this file runs as a script)
from mtets64_cases import MIN_BAND, ZERO_BAND, merged_bands
from oracle import texmlp as OT

RATIO = 3.0
H2_CEILING = 8.0
U = 2.0 ** -24
KINK, FACE = 2.0 ** -16, 1e-5
NUDGE = 5e-6          # lattice cases: a p placed on an integer is within 3e-6 of it (half an ulp of x_n times the scale 69) in float32 and float64; every other p is FACE away
# (group, tensor/route) -> (highest decades of the bands, bar, measured); h2 tensors only, bar = the largest measured figure x 1.5, below H2_CEILING.
# Both bands hold d(encoding) elements whose sum W1^T gz1 cancels to 1e-2 .. 1e-3 of its terms; the error keeps the size of the terms, 2^-21 of
# them in the h2 chain against 2^-24 in float32.
BAND_RATIO = {('magnitude', 'genc/3'): ((-4,), 7.3, 'MI355X 4.85, emulation 3.05 (409 elements)'),
              ('magnitude', 'genc/5'): ((-4,), 7.3, 'MI355X 4.85, emulation 3.05 (409 elements)'),
              ('mixed', 'genc@1e-2'): ((-7,), 5.1, 'MI355X 2.14, emulation 3.35 (788 elements)')}
MEASURED = {}
BANDS = {}            # (dev, group) -> {tensor: {decade: [count, sum (k - r64)^2, sum (r32 - r64)^2, sum r64^2]}}
DONE = {}
COMPLETE = set()
FRACTION = {}         # (dev, tag, tensor) -> largest |kernel - r64| / bound of the mixed-chain rule

LAY, TOTAL = OT.grid_layout()                  # [(scale, res, offset, size)], entries
f32c = lambda v: float(np.float32(v))
BOX = tuple(f32c(v) for v in (-0.8, -1.2, -0.2, 0.6, 0.6, 0.2))
FLIPPED = tuple(f32c(v) for v in (0.6, 0.6, 0.2, -0.8, -1.2, -0.2))            # mlptexture.py:94 (the reference's sign-flipped box, kept literally)
UNIT = (0.0, 0.0, 0.0, 1.0, 1.0, 1.0)
OMIN, OMAX = tuple(f32c(v) for v in (0, 0, 0, 0, 0.001, 0)), tuple(f32c(v) for v in (1, 1, 1, 0.5, 1, 1))
CAP_ENV = 'D3H_TEX_GRID_CAP'
H2_TENSORS = ('d_x', 'genc', 'd_table', 'd_w1', 'd_w2', 'd_w3')


def _seed(*a):
    return zlib.crc32('/'.join(str(x) for x in a).encode())


def _gen(*a):
    return torch.Generator().manual_seed(_seed(*a))


def _cdiv(a, b):
    return -(-a // b)


# ---- the op, restated ------------------------------------------------------------------------------------------------------------------------
class _ScaleGrad(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, s):
        ctx.s = s
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return g * ctx.s, None


def corners(xn, nudge=0.0):
    """per level: (fr [n,3], [index [n]] x 8) in the dtype of xn.  nudge (+-NUDGE, lattice cases): the cell is floor(p + nudge), so a p within
    NUDGE of an integer is put on the chosen side of the face and fr = p - floor extrapolates that cell: the one-sided derivative"""
    out = []
    for scale, res, off, size in LAY:
        p = xn * scale + 0.5
        fl = torch.floor(p + nudge)
        fr, pg = p - fl, fl.long()
        idx = []
        for c in range(8):
            i = (pg[:, 0] + (c & 1)) + (pg[:, 1] + ((c >> 1) & 1)) * res + (pg[:, 2] + ((c >> 2) & 1)) * res * res
            idx.append(torch.where(i >= size, i - size, i))
        out.append((fr, idx))
    return out


def encode(xn, tab2, nudge=0.0):
    """xn [n,3] in [0,1], tab2 [entries,2] -> [n,10]"""
    feats = []
    for (scale, res, off, size), (fr, idx) in zip(LAY, corners(xn, nudge)):
        lvl = tab2[off:off + size]
        acc = 0
        for c in range(8):
            w = 1.0
            for d in range(3):
                w = w * (fr[:, d] if (c >> d) & 1 else (1 - fr[:, d]))
            acc = acc + w[:, None] * lvl[idx[c]]
        feats.append(acc)
    return torch.cat(feats, -1)


def normalise(x, bbox):
    b0, b1 = x.new_tensor(bbox[:3]), x.new_tensor(bbox[3:])
    return (x - b0) / (b1 - b0)


def mlp(enc, w, gs):
    es = _ScaleGrad.apply(enc, gs) if gs != 1.0 else enc
    z1 = es @ w[0].t()
    z2 = torch.relu(z1) @ w[1].t()
    return z1, z2, torch.relu(z2) @ w[2].t()


def ref_eval(c, dtype, dev, kind, nudge=0.0):
    """kind 'mlp': out, enc, d_x, genc, d_table, d_w1..3 of sum(out G);  'enc': enc, d_x, d_table of sum(encode(xu) G10).  Masked pixels take
    no part (their rows are zero); the covered ones go through in chunks, whose parameter gradients autograd adds up."""
    n = c['n']
    act = torch.arange(n) if c['mask'] is None else torch.nonzero(c['mask'] > 0).reshape(-1)
    tab = c['table'].detach().clone().to(dev, dtype).requires_grad_(True)
    w = [t.detach().clone().to(dev, dtype).requires_grad_(True) for t in c['w']]
    r = {'enc': torch.zeros(n, 10, dtype=dtype), 'd_x': torch.zeros(n, 3, dtype=dtype)}
    if kind == 'mlp':
        r.update(out=torch.zeros(n, 6, dtype=dtype), genc=torch.zeros(n, 10, dtype=dtype))
        rng = torch.tensor(c['omax'], dtype=dtype, device=dev) - torch.tensor(c['omin'], dtype=dtype, device=dev)
        lo = torch.tensor(c['omin'], dtype=dtype, device=dev)
    for s in range(0, act.numel(), 1 << 16):
        idx = act[s:s + (1 << 16)]
        if kind == 'enc':
            xa = c['xu'][idx].clone().to(dev, dtype).requires_grad_(True)
            e = encode(xa, tab.view(-1, 2), nudge)
            (e * c['G10'][idx].to(dev, dtype)).sum().backward()
        else:
            xa = c['x'][idx].clone().to(dev, dtype).requires_grad_(True)
            e = encode(torch.clamp(normalise(xa, c['bbox']), 0, 1), tab.view(-1, 2), nudge)
            e.retain_grad()
            o = torch.sigmoid(mlp(e, w, c['gs'])[2]) * rng + lo
            (o * c['G'][idx].to(dev, dtype)).sum().backward()
            r['out'][idx] = o.detach().cpu()
            r['genc'][idx] = e.grad.cpu()
        r['enc'][idx] = e.detach().cpu()
        r['d_x'][idx] = xa.grad.cpu()
    r['d_table'] = (tab.grad if tab.grad is not None else torch.zeros_like(tab)).detach().cpu()
    if kind == 'mlp':
        for k, t in zip(('d_w1', 'd_w2', 'd_w3'), w):
            r[k] = (t.grad if t.grad is not None else torch.zeros_like(t)).detach().cpu().reshape(-1)
    return r


def refs(c, dev, kind):
    key = (torch.device(dev).type, kind)
    if key not in c['_ref']:
        c['_ref'][key] = (ref_eval(c, torch.float32, dev, kind), ref_eval(c, torch.float64, dev, kind))
    return c['_ref'][key]


def offenders(x, bbox, table, w, dev='cpu', lattice=False):
    """input hygiene in float64 -> bool [n]: a hidden pre-activation within KINK of its kink, or a p within FACE of an integer (lattice: unless
    it is within 3e-6 of it, where it was put on purpose)"""
    bad = torch.zeros(x.shape[0], dtype=torch.bool)
    tab, wd = table.to(dev, torch.float64).view(-1, 2), [t.to(dev, torch.float64) for t in w]
    with torch.no_grad():
        for s in range(0, x.shape[0], 1 << 17):
            xn = torch.clamp(normalise(x[s:s + (1 << 17)].to(dev, torch.float64), bbox), 0, 1)
            b = torch.zeros(xn.shape[0], dtype=torch.bool, device=xn.device)
            for scale, _, _, _ in LAY:
                p = xn * scale + 0.5
                dist = (p - torch.round(p)).abs()
                b |= ((dist < FACE) & ~((dist < 3e-6) & lattice)).any(-1)
            h = encode(xn, tab)
            for wl in wd[:2]:
                z = h @ wl.t()
                b |= (z.abs() < KINK * (h.abs() @ wl.abs().t())).any(-1)
                h = torch.relu(z)
            bad[s:s + (1 << 17)] = b.cpu()
    return bad


def counts(c, kind='mlp'):
    """[entries] number of (covered pixel with an upstream gradient, corner) pairs that address each table entry, float64 positions"""
    if ('_cnt', kind) in c:
        return c[('_cnt', kind)]
    cnt = c[('_cnt', kind)] = torch.zeros(TOTAL, dtype=torch.int64)
    live = covered(c) & ~((c['G10'] if kind == 'enc' else c['G']) == 0).all(-1)
    xn = torch.clamp(normalise(c['x'][live].double(), c['bbox']), 0, 1)
    for (scale, res, off, size), (fr, idx) in zip(LAY, corners(xn)):
        for i in idx:
            cnt.index_add_(0, off + i, torch.ones_like(i))
    return cnt


# ---- materials and cases ---------------------------------------------------------------------------------------------------------------------
_MAT = {}


def material(amp=0.5, w1s=1.0, w3s=1.0):
    """table uniform in +-amp (1e-4: the tcnn initialisation), the weights of check_texmlp; w1s / w3s scale the first / last layer"""
    key = (amp, w1s, w3s)
    if key not in _MAT:
        g = _gen('material')
        table = (torch.rand(2 * TOTAL, generator=g) * 2 - 1) * amp
        _MAT[key] = (table, [torch.randn(32, 10, generator=g) * 0.5 * w1s, torch.randn(32, 32, generator=g) * 0.3, torch.randn(6, 32, generator=g) * 0.3 * w3s])
    return _MAT[key]


def world(xn, bbox):
    b0, b1 = torch.tensor(bbox[:3]), torch.tensor(bbox[3:])
    return (b0 + xn * (b1 - b0)).float()


def draw(k, g, bbox, margin):
    """k points uniform over the box enlarged by `margin` of its size on every side (margin 0.1: 1 in 6 per axis is clamped)"""
    return world(torch.rand(k, 3, generator=g) * (1 + 2 * margin) - margin, bbox)


def make_case(tag, n, group, routes, *, mask=None, x=None, bbox=BOX, omin=OMIN, omax=OMAX, gs=128.0, mat=(), margin=0.1, G=None, G10=None,
              place=None, dev='cpu', cap=None, expect=None, lattice=False):
    """x None: random points, redrawn for hygiene; x given: prescribed positions, offenders masked.  place(x): points put somewhere on purpose
    after the redraw (they are then treated as prescribed).  G / G10: upstream gradients (default randn)."""
    g = _gen(tag)
    table, w = material(*mat)
    prescribed = x is not None
    if x is None:
        x = draw(n, g, bbox, margin)
        bad = offenders(x, bbox, table, w, dev)
        rounds = 0
        while bad.any():
            rounds += 1
            assert rounds <= 8 and int(bad.sum()) <= 0.05 * n + 1, (tag, 'hygiene: redraw', rounds, int(bad.sum()), n)
            idx = torch.nonzero(bad).reshape(-1)
            x[idx] = draw(idx.numel(), g, bbox, margin)
            bad[idx] = offenders(x[idx], bbox, table, w, dev)
    if place is not None:
        x, prescribed = place(x.clone()), True
    x = x.float().contiguous()
    if mask is not None:
        mask = mask.float().contiguous()
    if prescribed:
        bad = offenders(x, bbox, table, w, dev, lattice) & ((mask > 0) if mask is not None else torch.ones(n, dtype=torch.bool))
        assert int(bad.sum()) <= 0.02 * n, (tag, 'hygiene: more than 2 % of the prescribed positions offend', int(bad.sum()), n)
        if bad.any():
            mask = torch.ones(n) if mask is None else mask
            mask[bad] = 0.0
    G = torch.randn(n, 6, generator=g) if G is None else (G(g) if callable(G) else G)
    G10 = torch.randn(n, 10, generator=g) if G10 is None else (G10(g) if callable(G10) else G10)
    xu = torch.clamp(normalise(x, bbox), 0, 1)              # float32, operation for operation the kernel's x_n: the unit-box routes take it as x
    return dict(tag=tag, n=n, group=group, routes=routes, x=x, xu=xu.contiguous(), mask=mask, table=table, w=w, bbox=bbox, omin=omin, omax=omax, gs=float(gs),
                G=G.float().contiguous(), G10=G10.float().contiguous(), cap=cap, expect=expect or {}, lattice=lattice, _ref={})


_CASES = {}
ALL_BWD = ('wrap', 3, 4, 5, '5e', 6, 7, 8)
ALL = (1, 2) + ALL_BWD


def case(tag, dev='cpu'):
    s = dict(SPECS[tag])
    build, on_dev = s.pop('build'), s.pop('dev', False)
    key = (tag, torch.device(dev).type if on_dev else 'cpu')
    if key not in _CASES:
        _CASES[key] = build(tag, dev=dev, **s) if on_dev else build(tag, **s)
    return _CASES[key]


def _decades(shape, g, lo=-12, hi=2):
    return 10.0 ** torch.randint(lo, hi + 1, shape, generator=g).double()


def b_tail(tag, n, masked):
    g = _gen(tag, 'mask')
    mask = (torch.rand(n, generator=g) > 0.25).float() if masked else None
    if masked and n > 1:
        mask[0] = 1.0
    return make_case(tag, n, 'tails', (1, 2, 3, 7, 8), mask=mask)


def b_masks(tag, kind):
    n = 130 if kind == 'n130-all-masked' else 448
    g = _gen(tag, 'mask')
    if kind in ('all-masked', 'n130-all-masked'):
        mask = torch.zeros(n)
    elif kind == 'one-per-wave':
        mask = torch.zeros(n)
        mask[torch.arange(0, n, 64) + torch.randint(0, 64, (n // 64,), generator=g)] = 1.0
    elif kind == 'empty-chains':              # wave 0: first chain background, wave 1: second chain, wave 2: all, wave 3: none, then both again
        mask = torch.ones(n)
        mask[0:32] = 0
        mask[96:128] = 0
        mask[128:192] = 0
        mask[256:288] = 0
        mask[352:384] = 0
    elif kind == 'zero-gradient':
        mask = (torch.rand(n, generator=g) > 0.1).float()
    else:                                     # 'negative': mask values -1, -0.0, 0, 1e-30, 0.5, 2 -- covered means > 0
        vals = torch.tensor([-1.0, -0.0, 0.0, 1e-30, 0.5, 2.0])
        mask = vals[torch.randint(0, 6, (n,), generator=g)]
    expect, kw = ({'nothing': 'all'} if 'all-masked' in kind else {}), {}
    if kind == 'zero-gradient':
        # covered pixels WITHOUT an upstream gradient among live ones: wave 0 its first chain, wave 1 its second, wave 2 all of it, wave 3 none,
        # wave 4 every third pixel, wave 5 all but one pixel of each chain, wave 6 a single pixel; the 10-channel gradient of route 8 alike
        dead = torch.zeros(n, dtype=torch.bool)
        dead[0:32] = dead[96:128] = dead[128:192] = True
        dead[256:320:3] = True
        dead[320:384] = True
        dead[[325, 370]] = False
        dead[400] = True
        live = lambda width: (lambda gg: torch.randn(n, width, generator=gg) * (~dead)[:, None])
        kw, expect = dict(G=live(6), G10=live(10)), {'dead': int(dead.sum())}
    return make_case(tag, n, 'edges', ALL, mask=mask, expect=expect, **kw)


def b_box(tag, kind):
    n = 320
    g = _gen(tag, 'box')
    kw = dict(mask=(torch.rand(n, generator=g) > 0.15).float())
    if kind.startswith('outside'):
        def place(x, kind=kind):
            xn = torch.rand(n, 3, generator=g) * 0.9 + 0.05
            out = torch.where(torch.rand(n, 3, generator=g) < 0.5, -0.3 * torch.rand(n, 3, generator=g) - 0.01, 1.01 + 0.3 * torch.rand(n, 3, generator=g))
            axes = {'outside-x': [0], 'outside-y': [1], 'outside-z': [2], 'outside-xyz': [0, 1, 2]}[kind]
            sel = torch.rand(n, generator=g) < 0.6
            for d in axes:
                xn[sel, d] = out[sel, d]
            return world(xn, BOX)
        kw.update(place=place, expect={'clamped': True})
    elif kind == 'on-0-and-1':                # x exactly on the box faces: x_n == 0 / == 1 exactly, inside, the gradient passes
        def place(x):
            xn = torch.rand(n, 3, generator=g) * 0.9 + 0.05
            face = torch.randint(0, 3, (n, 3), generator=g)
            xn = torch.where(face == 0, torch.zeros(()), torch.where(face == 1, torch.ones(()), xn))
            xn[0], xn[1] = 0.0, 1.0
            return xn
        kw.update(place=place, bbox=UNIT, expect={'faces': True})
    elif kind == 'flipped':
        kw.update(bbox=FLIPPED)
    elif kind == 'gs1':
        kw.update(gs=1.0)
    elif kind == 'omax-eq-omin':
        kw.update(omin=tuple(f32c(v) for v in (0, 0.25, 0, 0, 0.001, 0)), omax=tuple(f32c(v) for v in (1, 0.25, 1, 0.5, 1, 1)))
    elif kind == 'ranges-zero':
        kw.update(omin=tuple(f32c(v) for v in (0.1, 0.2, 0.3, 0.4, 0.5, 0.6)), omax=tuple(f32c(v) for v in (0.1, 0.2, 0.3, 0.4, 0.5, 0.6)), expect={'nothing': 'mlp'})
    return make_case(tag, n, 'edges', ALL, **kw)


def cell_points(cells, g, level=4):
    """positions in the given cells (pg triples, [k,3]) of `level`, at random fractions 0.1 .. 0.9 of the cell"""
    scale = LAY[level][0]
    return (cells.double() + 0.1 + 0.8 * torch.rand(cells.shape[0], 3, generator=g).double() - 0.5) / scale


def scatter_layout():
    """hand-placed runs, one wave (64 lanes) each unless said otherwise -> (cells [n,3] at level 4, covered [n])"""
    A, B = torch.tensor([20, 30, 40]), torch.tensor([50, 12, 7])
    waves, cover = [], []

    def wave(runs, masked=()):
        cs = torch.cat([torch.as_tensor(c).reshape(1, 3).repeat(k, 1) for c, k in runs])
        assert cs.shape[0] == 64
        m = torch.ones(64)
        m[list(masked)] = 0
        waves.append(cs)
        cover.append(m)
    wave([(A, 64)])                                                                      # 64 lanes in one cell
    waves.append(torch.stack([torch.tensor([3 + 2 * (i % 8), 5 + 2 * (i // 8), 9]) for i in range(64)]))   # 64 distinct cells, no two face-adjacent
    cover.append(torch.ones(64))
    wave([(A, 21), (B, 22), (A, 21)])                                                    # A B A
    wave([(A, 31), (A, 1), (A, 32)], masked=(31,))                                       # A, masked, A
    for axis in range(3):
        for sign in (1, -1):
            e = torch.zeros(3, dtype=torch.long)
            e[axis] = sign
            wave([(A + k * e, 16) for k in range(4)])                                    # four face-adjacent runs in a row
            wave([(B + k * e, 21 + (k == 1)) for k in range(3)])                         # three
    wave([(A + torch.tensor([k, k, 0]), 16) for k in range(4)])                          # diagonal neighbours: no fold
    wave([(A + torch.tensor([k, k, k]), 16) for k in range(4)])
    wave([(B, 40), (A, 24)])                                                             # a run that ends at lane 63 ...
    wave([(A, 21), (B, 43)])                                                             # ... and continues in the next wave
    return torch.cat(waves), torch.cat(cover)


def b_scatter(tag, kind):
    g = _gen(tag, 'pos')
    if kind == 'runs':
        cells, cover = scatter_layout()
        xn = cell_points(cells, g)
    else:                                      # the coherent curve of check_texmlp
        from gridenc_cases import coherent_curve
        xn, cover = coherent_curve(1024).double(), torch.ones(1024)
    n = xn.shape[0]
    return make_case(tag, n, 'scatter', (3, 7, 8), x=world(xn, UNIT), mask=cover, bbox=UNIT, expect={'many': 8})


def shell_points(g, k=256):
    """x_n in the shell where corner indices reach res: per axis uniform above 0.9667 (level 0), 0.99957 (level 2), 0.99994 (level 3), or exactly 1"""
    lo = torch.tensor([0.9667, 0.99957, 0.99994, 1.0])[torch.randint(0, 4, (k, 3), generator=g)]
    xn = lo + (1 - lo) * torch.rand(k, 3, generator=g)
    xn[0] = 1.0                                # the corner (1, 1, 1)
    return xn.float()


def row_crossing(g):
    """level 0 (res 16): runs of 16 pixels in the cells (15, k, z) and (0, k + 1, z): cell difference 1, not spatially adjacent"""
    pts = []
    for k, z in ((3, 4), (9, 2), (14, 14), (15, 7)):
        for cx, cy in ((15, k), (0, k + 1), (15, k), (0, k + 1)):
            if cy > 15:
                cy = 15
            pts.append(cell_points(torch.tensor([[cx, cy, z]]).repeat(16, 1), g, level=0))
    return torch.cat(pts).clamp(0, 1).float()


def b_spill(tag, kind):
    g = _gen(tag, 'pos')
    xn = shell_points(g) if kind == 'shell' else row_crossing(g)
    return make_case(tag, xn.shape[0], 'spill', (1, 2, 3, 7, 8), x=xn, bbox=UNIT, expect={'spill': kind})


def b_lattice(tag):
    """points ON cell faces: per axis at random a lattice coordinate of level 0 (p = x_n 15 + 0.5 an integer: x_n = (2 j - 1) / 30), of level 4,
    or a generic one.  The forward is continuous there and is held to (a); d_x must be one of the two one-sided float64 derivatives."""
    n, g = 384, _gen(tag, 'pos')
    table, w = material()

    def points(k):
        xn = torch.rand(k, 3, generator=g).double() * 0.9 + 0.05
        kind = torch.randint(0, 3, (k, 3), generator=g)
        kind[:, 0][kind.sum(-1) == 0] = 1                                               # every point is on a face
        l0 = (2 * torch.randint(1, 16, (k, 3), generator=g).double() - 1) / 30
        l4 = (torch.randint(1, 69, (k, 3), generator=g).double() - 0.5) / LAY[4][0]
        return torch.where(kind == 1, l0, torch.where(kind == 2, l4, xn)).float()
    xn = points(n)
    bad, rounds = offenders(xn, UNIT, table, w, lattice=True), 0
    while bad.any():                                                                    # (the redraw of make_case, with new lattice points)
        rounds += 1
        assert rounds <= 8 and int(bad.sum()) <= 0.05 * n + 1, (tag, rounds, int(bad.sum()))
        idx = torch.nonzero(bad).reshape(-1)
        xn[idx] = points(idx.numel())
        bad[idx] = offenders(xn[idx], UNIT, table, w, lattice=True)
    return make_case(tag, n, 'lattice', (1, 2, 3, 7, 8), x=xn, bbox=UNIT, lattice=True)


def b_decades(tag):
    n = 2048
    return make_case(tag, n, 'magnitude', (3, 5, 7), G=lambda g: (torch.randn(n, 6, generator=g).double() * _decades((n // 32, 1, 1), g).expand(-1, 32, 6).reshape(n, 6)).float())


MIXED_LEVELS = (0, -2, -4, -6, -8)


def b_mixed(tag):
    n = 2048

    def G(g):
        lev = torch.tensor(MIXED_LEVELS)[torch.arange(n) % 5].double()
        base = torch.rand(n, 6, generator=g).double() * 0.5 + 0.5
        sign = torch.where(torch.rand(n, 6, generator=g) < 0.5, -1.0, 1.0).double()
        return (base * sign * (10.0 ** lev)[:, None] * _decades((n // 32, 1, 1), g, -6, 0).expand(-1, 32, 6).reshape(n, 6)).float()
    c = make_case(tag, n, 'mixed', (3,), G=G, margin=0.0)
    c['level'] = torch.tensor(MIXED_LEVELS)[torch.arange(n) % 5]
    return c


def b_range(tag, kind):
    mat = {'amp1e-4': (1e-4,), 'amp0.5': (0.5,), 'amp8': (8.0,), 'hidden1e3': (0.5, 2000.0, 1e-3)}[kind]
    return make_case(tag, 512, 'range', (1, 2, 3, 7, 8), mat=mat, mask=(torch.rand(512, generator=_gen(tag, 'mask')) > 0.2).float())


def tile_mask(n, grid, g, keep=0.35):
    """whole 256-pixel tiles empty: the first tile of every second workgroup of a `grid`-wide launch, and at random all but `keep` of the rest, so a
    persistent workgroup meets a covered tile after an empty one; inside a covered tile one pixel in five is background"""
    nt = _cdiv(n, 256)
    tiles = torch.rand(nt, generator=g) < keep
    tiles[:min(grid, nt):2] = False
    tiles[grid:min(2 * grid, nt):2] = True         # ... whose second tile is covered
    tiles[nt - 1] = True                           # the tail
    m = tiles.repeat_interleave(256)[:n].float() * (torch.rand(n, generator=g) > 0.2).float()
    m[n - 1] = 1.0
    return m


def b_loops(tag, n, grid, routes, cap=None, dev='cpu', keep=0.35):
    g = _gen(tag, 'mask')
    return make_case(tag, n, 'loops', routes, mask=tile_mask(n, cap or grid, g, keep), cap=cap, dev=dev)


SPECS = {}
for _n in (1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 511, 512, 513):
    for _m in (0, 1):
        SPECS[f'tail n{_n}' + (' mask' if _m else '')] = dict(build=b_tail, n=_n, masked=_m)
for _k in ('all-masked', 'n130-all-masked', 'one-per-wave', 'empty-chains', 'negative', 'zero-gradient'):
    SPECS[f'mask {_k}'] = dict(build=b_masks, kind=_k)
for _k in ('outside-x', 'outside-y', 'outside-z', 'outside-xyz', 'on-0-and-1', 'flipped', 'gs1', 'omax-eq-omin', 'ranges-zero'):
    SPECS[f'box {_k}'] = dict(build=b_box, kind=_k)
for _k in ('runs', 'curve'):
    SPECS[f'scatter {_k}'] = dict(build=b_scatter, kind=_k)
for _k in ('shell', 'rows'):
    SPECS[f'spill {_k}'] = dict(build=b_spill, kind=_k)
SPECS['lattice faces'] = dict(build=b_lattice)
SPECS['magnitude decades'] = dict(build=b_decades)
SPECS['mixed chains'] = dict(build=b_mixed)
for _k in ('amp1e-4', 'amp0.5', 'amp8', 'hidden1e3'):
    SPECS[f'range {_k}'] = dict(build=b_range, kind=_k)
SPECS['loops cap3 n3501'] = dict(build=b_loops, n=3501, grid=3, cap=3, routes=ALL, keep=0.6)
# the GPU leg, at the real caps (the emulation would take minutes); the float64 reference runs on the device as well
SPECS['loops fwd 2039'] = dict(build=b_loops, n=2039 * 256 + 3 * 256 + 77, grid=2039, routes=(1,), dev=True, keep=0.15)
SPECS['loops bwd 1021'] = dict(build=b_loops, n=1021 * 256 + 2 * 256 + 33, grid=1021, routes=('wrap', 3, 4, 5, '5e', 6, 7, 8), dev=True, keep=0.25)
SPECS['loops scatter 4093'] = dict(build=b_loops, n=4093 * 256 + 256 + 19, grid=4093, routes=(4, '5e', 6), dev=True, keep=0.08)
GPU_ONLY = ('loops fwd 2039', 'loops bwd 1021', 'loops scatter 4093')
GROUPS = ('tails', 'edges', 'scatter', 'spill', 'lattice', 'magnitude', 'mixed', 'range', 'loops')


_PREFIX = {'tail': 'tails', 'mask': 'edges', 'box': 'edges'}
group_of = lambda tag: _PREFIX.get(tag.split()[0], tag.split()[0])


def tags(group, dev='cpu'):
    """the cases of a group on a device: the capped ones on the emulation only, the ones at the real caps on the GPU only"""
    return [t for t in SPECS if group_of(t) == group and (t not in GPU_ONLY if dev == 'cpu' else SPECS[t].get('cap') is None)]


# ---- rule (a) --------------------------------------------------------------------------------------------------------------------------------
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


def _compare(dev, group, tag, tensor, k, r32, r64, report, pool=True):
    assert tuple(k.shape) == tuple(r64.shape) == tuple(r32.shape), (tag, tensor, tuple(k.shape), tuple(r64.shape))
    k, r32, r64 = (t.detach().cpu().double().reshape(-1).numpy() for t in (k, r32, r64))
    assert np.isfinite(k).all(), (tag, tensor, 'not finite')
    assert np.isfinite(r64).all() and np.isfinite(r32).all(), (tag, tensor, 'the reference is not finite')
    dk, d32 = k - r64, r32 - r64
    nk, n32, n64 = float(np.linalg.norm(dk)), float(np.linalg.norm(d32)), float(np.linalg.norm(r64))
    ratio = nk / n32 if n32 > 0 else (0.0 if nk == 0 else float('inf'))
    rel = (lambda v: v / n64) if n64 > 0 else (lambda v: v)
    alone = k.size >= MIN_BAND
    report(f'[tex64] {dev:4s} {tag:36s} {tensor:14s} e_k {rel(nk):.3e} e_32 {rel(n32):.3e} ratio {ratio:.2f}' +
           ('' if n64 > 0 else ' (|r64| = 0: absolute)') + ('' if alone else ' (pooled only)'))
    if pool and tag not in DONE.setdefault((dev, group, tensor), set()):
        DONE[(dev, group, tensor)].add(tag)
        _bands(dev, group, tensor, dk, d32, r64)
    if alone:
        assert nk <= RATIO * n32, (tag, tensor, nk, n32, ratio)


def band_bar(group, tensor, top):
    exc = BAND_RATIO.get((group, tensor))
    return exc[1] if exc is not None and top in exc[0] else RATIO


def _top_decades(acc):
    rows = [[[b], acc[b][0]] for b in sorted(acc)]
    i = 0
    while len(rows) > 1 and i < len(rows):
        if rows[i][1] >= MIN_BAND:
            i += 1
            continue
        j = i + 1 if i + 1 < len(rows) else i - 1
        rows[j] = [sorted(rows[j][0] + rows[i][0]), rows[j][1] + rows[i][1]]
        del rows[i]
    return [r[0][-1] for r in rows]


def check_bands(dev, group, report=print):
    acc = BANDS.get((dev, group))
    assert acc, f'no run of group {group} recorded on {dev}'
    worst = []
    for tensor in sorted(acc):
        merged, tops = merged_bands(acc[tensor]), _top_decades(acc[tensor])
        assert len(tops) == len(merged)
        for (label, (n, sk, s32, s64)), top in zip(merged, tops):
            ratio = (sk / s32) ** 0.5 if s32 > 0 else (0.0 if sk == 0 else float('inf'))
            den = s64 ** 0.5 if s64 > 0 else 1.0
            bar = band_bar(group, tensor, top)
            report(f'[tex64] {dev:4s} band {group:10s} {tensor:14s} |r64| in {label:18s} n {n:8d} e_k {sk ** 0.5 / den:.3e} e_32 {s32 ** 0.5 / den:.3e} ratio {ratio:.2f} bar {bar:g}')
            if bar != RATIO:
                MEASURED[(dev, group, tensor, label)] = ratio
            if n >= MIN_BAND and sk > bar ** 2 * s32:
                worst.append((tensor, label, n, ratio, bar))
    assert not worst, worst


# ---- the kernel, route by route ----------------------------------------------------------------------------------------------------------------
def _f6(v):
    import ctypes
    return (ctypes.c_float * 6)(*[float(a) for a in v])


class _env:
    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kw}
        for k, v in self.kw.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        return False


def _sync(dev):
    if dev != 'cpu':
        torch.cuda.synchronize()


def run_route(dev, c, route):
    """-> {tensor name: cpu tensor} as the kernel left them; 'out*' / 'd_x' / 'genc' start as NaN, 'd_table' / 'd_w' as -0.0"""
    from d3h import _lib as L, texmlp
    n = c['n']
    PLS, BASE = texmlp.PER_LEVEL_SCALE, texmlp.BASE_RES
    assert texmlp.grid_param_count() == 2 * TOTAL and c['table'].numel() == 2 * TOTAL
    x, xu, tab = c['x'].to(dev), c['xu'].to(dev), c['table'].to(dev)
    m = c['mask'].to(dev) if c['mask'] is not None else None
    wcat = torch.cat([t.reshape(-1) for t in c['w']]).to(dev)
    nan = lambda *s: torch.full(s, float('nan'), dtype=torch.float32, device=dev)
    negz = lambda k: torch.full((k,), -0.0, dtype=torch.float32, device=dev)
    box, lo, hi = _f6(c['bbox']), _f6(c['omin']), _f6(c['omax'])
    fwd = lambda xx, mm, ww, bb, o, e: L.call('texmlp_fwd', xx, mm, tab, ww, n, PLS, BASE, bb, lo, hi, o, e)
    bwd = lambda enc_only, g, dt, dw, dx, ge: L.call('texmlp_bwd', x, m, tab, wcat, n, PLS, BASE, box, lo, hi, c['gs'], enc_only, g, dt, dw, dx, ge)
    r = {}
    with _env(**{CAP_ENV: c['cap'], 'D3H_TEX_DX_FUSED': '0' if route == '5e' else None}):
        if route == 1:
            r['out'] = nan(n, 6)
            fwd(x, m, wcat, box, r['out'], None)
        elif route == 2:
            r['enc_unit'], r['out'], r['enc'] = nan(n, 10), nan(n, 6), nan(n, 10)
            fwd(xu, m, None, _f6(UNIT), None, r['enc_unit'])            # what grid_encode issues (with the case's mask on top)
            fwd(x, m, wcat, box, r['out'], r['enc'])
        elif route == 'wrap':
            a = [t.clone().to(dev).requires_grad_(True) for t in (c['x'], c['table'], *c['w'])]
            out = texmlp.texture_mlp(a[0], a[1], a[2], a[3], a[4], c['bbox'], c['omin'], c['omax'], mask=m, in_grad_scale=c['gs'])
            (out * c['G'].to(dev)).sum().backward()
            _sync(dev)
            r.update(out=out.detach(), d_x=a[0].grad, d_table=a[1].grad, d_w1=a[2].grad.reshape(-1), d_w2=a[3].grad.reshape(-1), d_w3=a[4].grad.reshape(-1))
        elif route == 8:
            G10 = c['G10'].to(dev)
            r['d_x'], r['d_table'] = nan(n, 3), negz(2 * TOTAL)
            L.call('texmlp_bwd', xu, m, tab, None, n, PLS, BASE, _f6(UNIT), None, None, 1.0, 1, G10, r['d_table'], None, r['d_x'], None)
        else:
            G = c['G'].to(dev)
            r['d_table'], dw = negz(2 * TOTAL), negz(wcat.numel())
            if route != 6:
                r['d_x'] = nan(n, 3)
            if route != 7:
                r['genc'] = nan(n, 10)
            if route == 3:
                bwd(0, G, None, dw, r['d_x'], r['genc'])
                bwd(1, r['genc'], r['d_table'], None, None, None)
            elif route == 4:
                bwd(0, G, r['d_table'], dw, r['d_x'], r['genc'])
            elif route == 5:
                bwd(0, G, None, dw, None, r['genc'])
                bwd(1, r['genc'], None, None, r['d_x'], None)
                bwd(1, r['genc'], r['d_table'], None, None, None)
            elif route == '5e':
                bwd(0, G, r['d_table'], dw, r['d_x'], r['genc'])
            elif route == 6:
                bwd(0, G, r['d_table'], dw, None, r['genc'])
            elif route == 7:
                bwd(0, G, r['d_table'], dw, r['d_x'], None)
            r['d_w'] = dw
            r['d_w1'], r['d_w2'], r['d_w3'] = dw[:320], dw[320:1344], dw[1344:]
        _sync(dev)
    return {k: v.detach().cpu() for k, v in r.items()}


def covered(c):
    return torch.ones(c['n'], dtype=torch.bool) if c['mask'] is None else c['mask'] > 0


def check_exact(c, route, k):
    """rule (c)"""
    tag, cov = c['tag'], covered(c)
    nothing = c['expect'].get('nothing') == 'all' or (c['expect'].get('nothing') == 'mlp' and route != 8)      # (route 8 does not see the output ranges)
    for name in ('out', 'enc', 'enc_unit', 'd_x'):
        if name in k:
            assert not torch.isnan(k[name]).any(), (tag, route, name, 'NaN left')
            assert (k[name][~cov] == 0).all(), (tag, route, name, 'rows of masked pixels are not zero')
    if 'd_x' in k:
        if route != 8:
            v = normalise(c['x'], c['bbox'])                       # float32, as the kernel
            clamped = (v < 0) | (v > 1)
            assert (k['d_x'][clamped] == 0).all(), (tag, route, 'd_x of a clamped coordinate')
            nograd = (c['G'] == 0).all(-1)
            if c['expect'].get('clamped'):
                assert int((clamped.any(-1) & cov).sum()) >= 32, (tag, 'fewer than 32 covered pixels are clamped')
        else:
            nograd = (c['G10'] == 0).all(-1)
        assert (k['d_x'][nograd] == 0).all(), (tag, route, 'd_x of a pixel without an upstream gradient')
        if c['expect'].get('dead'):
            assert int((nograd & cov).sum()) >= c['expect']['dead'] // 2 and int((~nograd & cov).sum()) >= 64, (tag, 'the case lost its dead or its live pixels')
    if 'genc' in k:
        assert not torch.isnan(k['genc'][cov]).any(), (tag, route, 'genc of a covered pixel not written')
        assert (k['genc'][cov & (c['G'] == 0).all(-1)] == 0).all(), (tag, route, 'genc of a covered pixel without an upstream gradient')
    if 'd_table' in k and route != 'wrap':
        untouched = counts(c, 'enc' if route == 8 else 'mlp') == 0
        bits = k['d_table'].view(-1, 2)[untouched]
        assert (bits == 0).all() and torch.signbit(bits).all(), (tag, route, 'd_table written where no covered pixel has a corner')
        if nothing:
            assert torch.signbit(k['d_table']).all() and (k['d_table'] == 0).all(), (tag, route, 'd_table touched although nothing contributes')
    if 'd_w' in k and nothing:
        assert torch.signbit(k['d_w']).all() and (k['d_w'] == 0).all(), (tag, route, 'd_w touched although nothing contributes')
    if nothing and 'd_x' in k:
        assert (k['d_x'] == 0).all(), (tag, route, 'd_x although nothing contributes')


def run_case(dev, tag, report=print):
    """every route of a case: rule (c), rule (a) per tensor, the bands pooled into the case's group; rule (d) where the routes are there"""
    c = case(tag, dev)
    group, got = c['group'], {}
    for route in c['routes']:
        k = got[route] = run_route(dev, c, route)
        check_exact(c, route, k)
        kind = 'enc' if route == 8 else 'mlp'
        r32, r64 = refs(c, dev, kind)
        cov = covered(c)
        if c['lattice'] and route not in (1, 2):
            check_one_sided(dev, c, route, kind, k['d_x'], r32['d_x'], report)
            continue
        for name, t in k.items():
            if name == 'd_w':
                continue
            rn = 'enc' if name == 'enc_unit' else name
            a, b32, b64 = t, r32[rn], r64[rn]
            if name == 'genc':
                a, b32, b64 = a[cov], b32[cov], b64[cov]
            if name == 'd_table' and route != 'wrap':
                # the entries nothing addresses were held to -0.0 bit for bit by (c), and r32 = r64 = 0 there: they add nothing to either norm
                hit = (counts(c, kind) > 0).repeat_interleave(2)
                a, b32, b64 = a[hit], b32[hit], b64[hit]
            if a.numel() == 0:
                continue
            # (mixed chains: the per-pixel tensors and the table are pooled per gradient level only, check_mixed)
            _compare(dev, group, tag, f'{name}/{route}', a.reshape(b64.shape), b32, b64, report, pool=group != 'mixed' or name.startswith('d_w'))
        if c['expect'].get('many') and 'd_table' in k:
            cnt = counts(c, kind)
            big = (cnt >= c['expect']['many']).repeat_interleave(2) & (k['d_table'] != 0)
            assert big.any(), (tag, route, 'no table entry of many contributions')
    if 3 in got and 4 in got:
        assert torch.equal(got[3]['d_x'].view(torch.int32), got[4]['d_x'].view(torch.int32)), (tag, 'rule (d): d_x of routes 3 and 4 differ')
    if tag == 'mixed chains':
        check_mixed(dev, c, got[3], report)
    if c['expect'].get('spill'):
        check_spill(c)
    if c['expect'].get('faces'):
        v = normalise(c['x'], c['bbox'])
        on = ((v == 0) | (v == 1)) & covered(c)[:, None]
        assert int(on.sum()) >= 100 and (got[3]['d_x'][on] != 0).any(), (tag, 'no point on x_n == 0 / 1, or no gradient through them')
    COMPLETE.add((dev, group, tag))
    return got


def check_one_sided(dev, c, route, kind, k, r32, report):
    """lattice cases: every component of d_x is the derivative of the cell on one side of the face or of the other (the tangential derivatives
    are continuous across a face, so the choice is per component), to (a)'s bar: kernel and float32 reference each against the nearer one"""
    key = (torch.device(dev).type, kind, 'sides')
    if key not in c['_ref']:
        c['_ref'][key] = [ref_eval(c, torch.float64, dev, kind, s)['d_x'] for s in (NUDGE, -NUDGE)]
    rp, rm = c['_ref'][key]
    assert int((rp != rm).sum()) >= c['n'] // 2, (c['tag'], 'the two sides hardly differ: no point is on a face')
    near = lambda t: torch.minimum((t.double() - rp).abs(), (t.double() - rm).abs())
    nk, n32 = float(near(k).norm()), float(near(r32).norm())
    report(f'[tex64] {dev:4s} {c["tag"]:36s} {"d_x/" + str(route):14s} one-sided: e_k {nk / float(rp.norm()):.3e} e_32 {n32 / float(rp.norm()):.3e} ratio {nk / n32:.2f}')
    assert nk <= RATIO * n32, (c['tag'], route, 'd_x is neither one-sided derivative', nk, n32)


def check_spill(c):
    """the case does what it claims: corner indices reach res on levels 0, 2, 3, some spill into the next row and some wrap past the level's size"""
    xn = c['xu'].double()
    reach, wrap = set(), set()
    for l, (scale, res, off, size) in enumerate(LAY):
        pg = torch.floor(xn * scale + 0.5).long()
        if ((pg + 1) >= res).any():
            reach.add(l)
        raw = (pg[:, 0] + 1) + (pg[:, 1] + 1) * res + (pg[:, 2] + 1) * res * res
        if (raw >= size).any():
            wrap.add(l)
    if c['expect']['spill'] == 'shell':
        assert reach == {0, 2, 3} and wrap == {0, 2, 3}, (reach, wrap)
    else:
        pg = torch.floor(xn * LAY[0][0] + 0.5).long()
        cell = pg[:, 0] + pg[:, 1] * 16 + pg[:, 2] * 256
        d = cell[1:] - cell[:-1]
        assert int(((d.abs() == 1) & ((pg[1:, 1] - pg[:-1, 1]).abs() == 1)).sum()) >= 8, 'no run crosses from pg_x = res - 1 into the next row'


def check_mixed(dev, c, k, report):
    """module docstring, `Mixed chains`"""
    r32, r64 = refs(c, dev, 'mlp')
    lev, n = c['level'], c['n']
    for name in ('genc', 'd_x'):
        for L_ in (0, -2, -4):
            sel = lev == L_
            _compare(dev, 'mixed', c['tag'], f'{name}@1e{L_}', k[name][sel], r32[name][sel], r64[name][sel], report)
    w1, w2, w3 = (t.double().abs() for t in c['w'])
    with torch.no_grad():
        xn = torch.clamp(normalise(c['x'].double(), c['bbox']), 0, 1)
        o = mlp(encode(xn, c['table'].double().view(-1, 2)), [t.double() for t in c['w']], 1.0)[2]
        sg = torch.sigmoid(o)
        go = c['G'].double() * (torch.tensor(c['omax']).double() - torch.tensor(c['omin']).double()) * sg * (1 - sg)
    gmax = go.abs().reshape(n // 32, -1).max(1).values
    S = 2.0 ** (6 - torch.frexp(gmax)[1]).double()                                    # d3h_h2_pow2_scale
    S = S.repeat_interleave(32)[:, None]
    d = 2.0 ** -35
    A = ((torch.full((n, 6), d, dtype=torch.float64) @ w3 + d) @ w2 + d) @ w1                 # [n,10]
    R = ((go.abs() * S) @ w3) @ w2 @ w1
    bound = c['gs'] / S * (A + 8 * U * R)
    # the Jacobian d enc_c / d x of the float64 reference
    xa = c['x'].double().requires_grad_(True)
    e = encode(torch.clamp(normalise(xa, c['bbox']), 0, 1), c['table'].double().view(-1, 2))
    J = torch.stack([torch.autograd.grad(e[:, ch].sum(), xa, retain_graph=True)[0] for ch in range(10)], 1)      # [n,10,3]
    bound_x = (J.abs() * bound[:, :, None]).sum(1)
    for L_ in (-6, -8):
        sel = lev == L_
        for name, b in (('genc', bound), ('d_x', bound_x)):
            err = (k[name][sel].double() - r64[name][sel]).abs()
            frac = float((err / b[sel]).max())
            FRACTION[(dev, c['tag'], f'{name}@1e{L_}')] = frac
            rel = float((err / r64[name][sel].abs().clamp_min(1e-300)).median())
            report(f'[tex64] {dev:4s} {c["tag"]:36s} {name}@1e{L_} largest fraction of the subnormal-step bound {frac:.4f}; median relative error {rel:.3e}')
            assert frac <= 1.0, (c['tag'], name, L_, frac)


def check_group(dev, group, report=print):
    for tag in tags(group, dev):
        if (dev, group, tag) not in COMPLETE:
            run_case(dev, tag, lambda s: None)
    check_bands(dev, group, report)


def check_inputs():
    """the inputs have the edges they claim (host only)"""
    for n, masked in ((1, 0), (513, 1)):
        assert case(f'tail n{n}' + (' mask' if masked else ''))['n'] == n
    cells, cover = scatter_layout()
    assert cells.shape[0] % 64 == 0 and int((cover == 0).sum()) == 1
    c = case('scatter runs')
    assert int((counts(c) >= 64).sum()) >= 8                      # 64 lanes in one cell: its 8 entries hold 64 contributions each
    c = case('mask negative')
    assert (c['mask'] < 0).any() and (c['mask'] > 0).any() and (c['mask'] == 0).any()
    c = case('mixed chains')
    assert sorted(set(c['level'].tolist())) == sorted(MIXED_LEVELS)
    c = case('loops cap3 n3501')
    tiles = torch.nn.functional.pad(c['mask'], (0, (-c['n']) % 256)).reshape(-1, 256).sum(1) > 0
    assert not tiles[0] and tiles[3] and not tiles[2] and tiles[5], tiles                  # an empty first tile, a covered second one
    for tag in ('spill shell', 'spill rows'):
        check_spill(case(tag))


def main(dev):
    """every case with the figures as markdown tables on stdout; a missed bar is printed in bold and the run goes on"""
    import time
    lines, bands = [], []
    t0 = time.time()

    def attempt(what, f, *a):
        try:
            f(*a)
        except AssertionError as e:
            print(f'**bar missed in {what}: {str(e)[:400]}**\n')

    if dev == 'cpu':
        attempt('inputs', check_inputs)
    for g in GROUPS:
        for tag in tags(g, dev):
            attempt(tag, run_case, dev, tag, lines.append)
    for g in GROUPS:
        attempt(f'bands of group {g}', check_bands, dev, g, bands.append)
    print(f'# The grid encoding and texture MLP of csrc/texmlp.hip against float64 on ' + ('the host emulation' if dev == 'cpu' else 'one MI355X') + '\n')
    print(f'`python tests/tex64_cases.py {dev}`; rules, references and cases: the docstring of `tests/tex64_cases.py`.  `e_k` and `e_32` are the L2 distances of the '
          f'kernel and of the float32 reference from float64, relative to the float64 norm; tensors are named `tensor/route`.  {len([t for g in GROUPS for t in tags(g, dev)])} cases, '
          f'every run, reference and table: {time.time() - t0:.0f} s of host time.\n')
    print('## Exceptions to the ratio 3\n')
    for (g, t), (tops, bar, note) in BAND_RATIO.items():
        here = ', '.join(f'{r:.2f}' for (d_, g_, t_, lab), r in MEASURED.items() if (d_, g_, t_) == (dev, g, t))
        print(f'- group `{g}`, tensor `{t}`, band {" and ".join("1e%d" % d for d in tops)}: bar {bar}.  Measured in this run: {here}.  When the bar was set: {note}')
    if not BAND_RATIO:
        print('none: every tensor of every run and every pooled band meets 3, the h2 tensors included; no band is held to rule (b).')
    print('\n## Mixed chains: pixels 1e-6 and 1e-8 below their chain\'s largest gradient (asserted: fraction <= 1)\n')
    for s in lines:
        if 'subnormal-step bound' in s:
            print('- ' + ' '.join(s.split()[4:]))
    print('\n## One-sided derivatives at lattice points (asserted: ratio <= 3)\n')
    for s in lines:
        if 'one-sided' in s:
            print('- ' + ' '.join(s.split()[2:]))
    # condensed: per group and tensor over its routes and bands; every band at more than 2/3 of its bar in full
    rows = []
    for s in bands:
        w = s.split()
        i = w.index('n')
        tensor, _, route = w[4].partition('/')
        rows.append((w[3], tensor, route, ' '.join(w[7:i]), int(w[i + 1]), float(w[i + 3]), float(w[i + 5]), float(w[i + 7]), float(w[i + 9])))
    print('\n## Rule (a) per decade band of |float64 value|, pooled over the runs of a group (asserted: ratio <= bar in every band of >= 64 elements)\n')
    print('| group | tensor | routes | bands | elements | largest band ratio | in band | of route | bar there |\n|---|---|---|---|---|---|---|---|---|')
    per = {}
    for g, t, r, lab, n, ek, e32, ratio, bar in rows:
        row = per.setdefault((g, t), [set(), 0, 0, -1.0, '', '', 0.0])
        row[0].add(r)
        row[1] += 1
        row[2] += n
        if ratio > row[3] and n >= MIN_BAND:
            row[3:] = [ratio, lab, r, bar]
    for (g, t), (rs, nb, n, ratio, lab, r, bar) in per.items():
        print(f'| {g} | {t} | {" ".join(sorted(rs)) or "-"} | {nb} | {n} | {ratio:.2f} | {lab} | {r or "-"} | {bar:g} |')
    print('\nEvery band above two thirds of its bar:\n\n| group | tensor/route | band | elements | e_k | e_32 | ratio | bar |\n|---|---|---|---|---|---|---|---|')
    for g, t, r, lab, n, ek, e32, ratio, bar in rows:
        if n >= MIN_BAND and ratio > 2 * bar / 3:
            print(f'| {g} | {t}{"/" + r if r else ""} | {lab} | {n} | {ek:.3e} | {e32:.3e} | {ratio:.2f} | {bar:g} |')
    print('\n## Rule (a) per tensor of a run: the largest ratio over the runs of a group (asserted per run: ratio <= 3 for tensors of >= 64 elements)\n')
    print('| group | tensor | routes | comparisons | largest ratio | in run | of route | largest e_k |\n|---|---|---|---|---|---|---|---|')
    per = {}
    for s in lines:
        if ' e_k ' in s and 'one-sided' not in s:
            head, tail = s.split(' e_k ')
            w, t = head.split(), tail.split()
            tag = ' '.join(w[2:-1])
            tensor, _, route = w[-1].partition('/')
            row = per.setdefault((group_of(tag), tensor), [set(), 0, -1.0, '', '', 0.0])
            row[0].add(route)
            row[1] += 1
            if float(t[4]) > row[2]:
                row[2:5] = [float(t[4]), tag, route]
            row[5] = max(row[5], float(t[0]))
    for (g, name), (rs, k, ratio, run, r, ek) in per.items():
        print(f'| {g} | {name} | {" ".join(sorted(rs)) or "-"} | {k} | {ratio:.2f} | {run} | {r or "-"} | {ek:.3e} |')


if __name__ == '__main__':
    import sys
    import conftest
    from d3h import _lib as L
    device = sys.argv[1] if len(sys.argv) > 1 else 'cpu'
    if device == 'cpu':
        L._use_emulator_for_tests(conftest.EMUL_SO)
    main(device)
