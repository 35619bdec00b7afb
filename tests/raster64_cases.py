"""The position-gradient kernels of csrc/raster.hip (raster_bwd_kernel and its fold inside gbuffer_bwd_kernel, aa_bwd_kernel and its fused twin
aa_composite_bwd_kernel) against oracle/raster.py evaluated in FLOAT64, at pixel coordinates up to 4096; and the edges of the two antialias
kernels.  Shared by tests/test_raster64_emul.py (host emulation) and tests/test_gpu_raster64.py (MI355X).

The reference.  oracle/raster.py with torch's default dtype switched to float64 (oracle.fl) and float64 inputs: the same formulas and the SAME
DISCRETE DECISIONS as its float32 run -- OR.rasterize takes the winners through `ids=`, OR.antialias takes every decision from the float32
numpy copy of `pos` and does only the differentiable arithmetic in the dtype of `pos` / `color`.  Per compared tensor and case:
    e_k  = |kernel - float64|_2 / |float64|_2        e_32 = |float32 oracle - float64|_2 / |float64|_2       (and the max-norm versions, printed)
and THE BAR: over the large cases RMS(e_k) <= 3 RMS(e_32), per tensor; the same over the 48 x 48 controls.  The kernel may be three times as
far from float64 as the float32 restatement of the same formulas is -- measured against the reference's own distance from float64, never
against an earlier output of the kernel, and without an absolute floor.  (Measured, on the MI355X and under emulation alike:
1.00 for the rasterize chains, 1.2 - 1.4 for the antialias d_pos, at most 2.65 for one of the sums; profiles/raster64_gpu.md, raster64_emul.md.)

Large coordinates on a small frame.  window(): the 48 x 48 scene of the per-kernel suite squeezed into a 48 x 48 pixel window in the far corner
of a 48 x 4096 (large x) or 4096 x 48 (large y) frame: pixel coordinates of up to 4096 on 196 608 pixels (the oracle is a Python loop over
pixels).  Sub-pixel jitters from a fixed seed; half of the large cases sit a few hundred pixels away from the border.

Kinks.  The blend weight is |d - 0.5| and a pair exists for 0 <= d <= 1.  A pair whose float64 d is within 2e-3 of 0.5, 0 or 1 may sit on the
other side in float32 (the float32 error of d at coordinate 4096 is a few 1e-4): source and destination swap, an O(0.1) change of d_pos on
every float32 side and an error of none.  Before any backward the upstream gradient is zeroed on both pixels of every such pair (in all three
runs alike), those pixels are left out of the forward comparison, and at most 2 % of the pairs of a case may be dropped.  JITTER_SEED is
chosen so that the reference alone satisfies this on every case.

The cancelling sums.  Per d_pos tensor also s = sum_v d_pos[v, :2] . (ndc_v - centroid) w_v (the derivative of the loss under scaling the mesh
about its screen centroid: a bias along the silhouette normal survives this sum, rounding noise does not) and the plain sum of d_pos[..., :2]
over the vertices, with the same rule: RMS over the cases of |s_k - s_64| / |s_64| <= 3 x the same of the float32 oracle.  For these two sums to
mean something they must not cancel to nothing by themselves, so every chain takes a sign-coherent upstream gradient: the rasterize chains
interpolate a radial-plus-linear screen function under positive weights (_raster_inputs), the separate and fused antialias chains take a
positively weighted energy loss on a bright-on-dark image (_losses), the mask chain the product's squared error.
"""
import contextlib
import zlib

import numpy as np
import torch

from parity_cases import T, _raster_scene

WIN = 48
KINK = 2e-3
MAX_DROPPED = 0.02
RATIO = 3.0
JITTER_SEED = 24          # the first seed of 0, 1, 2, ... whose float64 reference keeps the 2 % cap on every case (it drops no pair at all)

# name: (H, W, pixels away from the far border along the long axis, frames, shared [1, V, 4] pos)
LARGE = {'x0': (48, 4096, 0, 1, False), 'x1': (48, 4096, 0, 2, False), 'x2': (48, 4096, 301, 1, False), 'x3': (48, 4096, 517, 1, False),
         'y0': (4096, 48, 0, 1, False), 'y1': (4096, 48, 0, 2, True), 'y2': (4096, 48, 411, 1, False), 'y3': (4096, 48, 250, 1, False)}
CONTROL = {'c0': (48, 48, 0, 1, False), 'c1': (48, 48, 0, 2, False)}
CASES = {**LARGE, **CONTROL}


def window(H, W, win=WIN, corner=(1.0, 1.0), jitter=(0.0, 0.0), nb=1):
    """_raster_scene(win, nb) mapped into a win x win pixel window of an H x W frame: clip x -> x win/W + (corner_x (1 - win/W) + jx 2/W) w (y
    likewise with H); corner +-1 picks the border, jitter is in pixels"""
    posn, f = _raster_scene(win, nb)
    p = posn.astype(np.float64)
    w = p[..., 3]
    out = p.copy()
    out[..., 0] = p[..., 0] * (win / W) + (corner[0] * (1.0 - win / W) + jitter[0] * 2.0 / W) * w
    out[..., 1] = p[..., 1] * (win / H) + (corner[1] * (1.0 - win / H) + jitter[1] * 2.0 / H) * w
    return out.astype(np.float32), f


def case_scene(name):
    """-> posn [nb or 1, V, 4] float32, faces, H, W, nb"""
    H, W, away, nb, shared = CASES[name]
    jit = np.random.default_rng(JITTER_SEED).uniform(-0.5, 0.5, (len(CASES), 2))[list(CASES).index(name)]
    jx = jit[0] - (away if W > H else 0)
    jy = jit[1] - (away if H > W else 0)
    posn, f = window(H, W, jitter=(jx, jy), nb=1 if shared else nb)
    return posn, f, H, W, nb


def _gen(name, salt):
    return torch.Generator().manual_seed(zlib.crc32(f'{name}/{salt}'.encode()))


@contextlib.contextmanager
def _default_dtype(dt):
    old = torch.get_default_dtype()
    torch.set_default_dtype(dt)
    try:
        yield
    finally:
        torch.set_default_dtype(old)


def _err(a, ref, keep=None):
    a, ref = a.detach().cpu().double(), ref.detach().double()
    if keep is not None:
        a, ref = a * keep, ref * keep
    d = a - ref
    return float(d.norm() / ref.norm()), float(d.abs().max() / ref.abs().max())


def _sums(dp, posn):
    """(dilation derivative, plain sum over the vertices [2]) of d_pos, in float64"""
    p = torch.from_numpy(posn).double()
    dp = dp.detach().cpu().double()
    ndc = p[..., :2] / p[..., 3:]
    s = (dp[..., :2] * (ndc - ndc.mean(1, keepdim=True)) * p[..., 3:]).sum()
    return s, dp[..., :2].sum((0, 1))


RESULTS = {}          # (dev, case) -> {'tensors': {name: (e_k, e_32, max_k, max_32)}, 'sums': {name: (dil_k, dil_32, sum_k, sum_32, s_64)}}
_REF = {}


def _record(dev, name, tensor, got, r32, r64, keep=None, posn=None):
    res = RESULTS.setdefault((dev, name), {'tensors': {}, 'sums': {}})
    ek, mk = _err(got, r64, keep)
    e32, m32 = _err(r32, r64, keep)
    assert np.isfinite(ek) and np.isfinite(e32), (name, tensor, ek, e32)
    res['tensors'][tensor] = (ek, e32, mk, m32)
    print(f'[raster64] {dev:4s} {name} {tensor:22s} L2 kernel {ek:.3e} oracle32 {e32:.3e} | max kernel {mk:.3e} oracle32 {m32:.3e}')
    if posn is not None:
        (sk, tk), (s32, t32), (s64, t64) = _sums(got, posn), _sums(r32, posn), _sums(r64, posn)
        row = (float((sk - s64).abs() / s64.abs()), float((s32 - s64).abs() / s64.abs()),
               float((tk - t64).norm() / t64.norm()), float((t32 - t64).norm() / t64.norm()), float(s64))
        res['sums'][tensor] = row
        print(f'[raster64] {dev:4s} {name} {tensor:22s} dilation s64 {row[4]:+.4e} kernel {row[0]:.3e} oracle32 {row[1]:.3e} | vertex sum kernel {row[2]:.3e} '
              f'oracle32 {row[3]:.3e}')


# ---- rasterize backward, alone and folded into the G-buffer's -----------------------------------------------------------------------------
def _rho(name):
    """per frame of `pos`: the vertices' screen offsets from the mesh's centroid in units of the window, [P, V, 2] float64, and the centroid in pixels"""
    posn, f, H, W, nb = case_scene(name)
    p = torch.from_numpy(posn).double()
    ndc = p[..., :2] / p[..., 3:]
    c = ndc.mean(1, keepdim=True)
    half = torch.tensor([W / 2.0, H / 2.0], dtype=torch.float64)
    return (ndc - c) * half / WIN, (c[:, 0] + 1.0) * half


def _pixel_weight(name):
    """[nb, H, W, 1] float32 in (0.1, 2): 1 + (offset of the pixel from the mesh's centroid, x + y, in windows): a loss weighted by it changes
    under a TRANSLATION of the mesh with one sign (the side with the larger weight wins), so the plain vertex sum of d_pos does not cancel"""
    posn, f, H, W, nb = case_scene(name)
    _, cpix = _rho(name)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64) + 0.5, torch.arange(W, dtype=torch.float64) + 0.5, indexing='ij')
    w = torch.stack([1.0 + ((xs - cpix[b if cpix.shape[0] > 1 else 0, 0]) + (ys - cpix[b if cpix.shape[0] > 1 else 0, 1])) / WIN for b in range(nb)])
    return w.clamp(0.1, 2.0).float()[..., None]


def _raster_inputs(name):
    """Sign-coherent upstream gradients (module docstring, "The cancelling sums").  The interpolated quantity is phi = |rho|^2 + rho_x + rho_y of
    the vertex's screen offset rho from the centroid: at a fixed pixel it FALLS when the mesh is scaled up about the centroid (by 2 |rho|^2, the
    linear part cancels over the mesh) and when the mesh moves along (1, 1) (by 1 per pixel), so with positive per-pixel weights neither the
    dilation derivative nor the vertex sum of d_pos cancels.  attr: three affine images of phi; the weights are 0.5 + uniform."""
    posn, f, H, W, nb = case_scene(name)
    g = _gen(name, 'raster')
    Fn = f.shape[0]
    rho, _ = _rho(name)
    phi = ((rho ** 2).sum(-1) + rho.sum(-1)).float()                                   # [P, V]
    attr = torch.stack([phi + 0.3, 2.0 * phi - 0.2, 0.5 * phi + 0.1], -1)
    return {'phi': phi, 'k': 0.5 + torch.rand(nb, H, W, 1, generator=g), 'attr': attr, 'face': torch.randn(nb, Fn, 3, generator=g),
            'G0': 0.5 + torch.rand(nb, H, W, 3, generator=g), 'G1': torch.randn(nb, H, W, 3, generator=g)}


def _uv_upstream(name, ids, inp):
    """d(sum_p k_p phi(p)) / d(u, v) for the winners `ids`: k (phi_0 - phi_2, phi_1 - phi_2) of the pixel's triangle, 0 where nothing is covered"""
    posn, f, H, W, nb = case_scene(name)
    tv = torch.from_numpy(f)[(ids.long() - 1).clamp(min=0)]                             # [nb, H, W, 3]
    phi = inp['phi'].expand(nb, -1)
    ph = torch.stack([phi[b][tv[b]] for b in range(nb)])                              # [nb, H, W, 3]
    G = torch.stack([ph[..., 0] - ph[..., 2], ph[..., 1] - ph[..., 2]], -1) * inp['k']
    return G * (ids > 0)[..., None]


def _raster_reference(name, ids):
    """float32 and float64 oracle with the winners `ids`: (u, v), rast_db, d_pos of sum(G (u, v)), d_pos through interpolate (the fold)"""
    key = ('raster', name, zlib.crc32(ids.numpy().tobytes()))
    if key in _REF:
        return _REF[key]
    from oracle import raster as OR
    posn, f, H, W, nb = case_scene(name)
    inp = _raster_inputs(name)
    inp['G'] = _uv_upstream(name, ids, inp)
    tri_o = torch.from_numpy(f)
    fidx = torch.arange(f.shape[0])[:, None].expand(-1, 3).contiguous()
    out = {}
    for dt in (torch.float32, torch.float64):
        with _default_dtype(dt):
            pos = torch.from_numpy(posn).to(dt).requires_grad_(True)
            rast, db = OR.rasterize(pos.expand(nb, -1, -1), tri_o, H, W, ids=ids)
            d_pos, = torch.autograd.grad((rast[..., :2] * inp['G'].to(dt)).sum(), pos, retain_graph=True)
            img, _ = OR.interpolate(inp['attr'].to(dt), rast, tri_o)
            fimg, _ = OR.interpolate(inp['face'].to(dt), rast, fidx)
            d_fold, = torch.autograd.grad((img * inp['G0'].to(dt)).sum() + (fimg * inp['G1'].to(dt)).sum(), pos)
        out[dt] = {'uv': rast[..., :2].detach(), 'db': db.detach(), 'd_pos': d_pos, 'fold.d_pos': d_fold}
    _REF[key] = out
    return out


def run_raster(dev, name):
    if 'rast.uv' in RESULTS.get((dev, name), {'tensors': {}})['tensors']:
        return RESULTS[(dev, name)]
    from d3h import raster
    posn, f, H, W, nb = case_scene(name)
    inp = _raster_inputs(name)
    tri = T(f.astype(np.int32), dev)
    got = {}
    old = raster.BIN_MIN_TRIS
    try:
        for binned in (False, True):
            raster.BIN_MIN_TRIS = 1 if binned else 1 << 30
            pos = T(posn, dev, True)
            rast, db = raster.rasterize(pos, tri, (H, W), nb=nb)
            G = _uv_upstream(name, rast.detach()[..., 3].cpu(), inp)
            (rast[..., :2] * G.to(dev)).sum().backward()
            got[binned] = (rast.detach().cpu(), db.detach().cpu(), pos.grad.cpu())
    finally:
        raster.BIN_MIN_TRIS = old
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1]), 'the two rasterisers differ'
    ids = got[0][0][..., 3]
    assert (ids > 0).float().mean() * (H * W) > 0.05 * WIN * WIN
    # the fold: rasterize -> gbuffer(raster_pos=), one attribute group and a face attribute
    pos = T(posn, dev, True)
    rs, _ = raster.rasterize(pos, tri, (H, W), nb=nb)
    groups, fimg, _ = raster.gbuffer(inp['attr'].to(dev), (3,), rs, tri, face_attr=inp['face'].to(dev), want_mask=True, raster_pos=pos)
    ((groups[0] * inp['G0'].to(dev)).sum() + (fimg * inp['G1'].to(dev)).sum()).backward()
    ref = _raster_reference(name, ids)
    r32, r64 = ref[torch.float32], ref[torch.float64]
    _record(dev, name, 'rast.uv', got[0][0][..., :2], r32['uv'], r64['uv'])
    _record(dev, name, 'rast.db', got[0][1], r32['db'], r64['db'])
    _record(dev, name, 'rast.d_pos', got[0][2], r32['d_pos'], r64['d_pos'], posn=posn)
    _record(dev, name, 'rast.d_pos(binned)', got[1][2], r32['d_pos'], r64['d_pos'], posn=posn)
    _record(dev, name, 'fold.d_pos', pos.grad, r32['fold.d_pos'], r64['fold.d_pos'], posn=posn)
    return RESULTS[(dev, name)]


# ---- antialias: separate, fused with six source kinds, the mask chain ----------------------------------------------------------------------
COMP_ZERO, COMP_IMAGE, COMP_CONST20, COMP_ALPHA = 0, 1, 2, 3


def ref_composite(rast, sources):
    """render.py:375-382,430-449 per buffer as torch ops in the dtype of the sources (tests/parity_cases.py:check_composite): lerp(background,
    [values, 1], coverage); COMP_ALPHA: the value is the alpha, one channel"""
    B, H, W = rast.shape[:3]
    outs = []
    for vals, kind, bg in sources:
        vals = vals.expand(B, H, W, vals.shape[-1])
        cov = (rast[..., 3:] > 0).to(vals.dtype)
        if kind == COMP_ALPHA:
            outs.append(torch.lerp(torch.zeros_like(vals), torch.ones_like(vals), cov * vals))
            continue
        buf = torch.cat((vals, torch.ones_like(vals[..., :1])), -1)
        if kind == COMP_IMAGE:
            bg = bg.to(vals.dtype).expand(B, H, W, 3)
            b_ = torch.cat((bg, torch.zeros_like(bg[..., :1])), -1)
        else:
            b_ = torch.full_like(buf, 20.0) if kind == COMP_CONST20 else torch.zeros_like(buf)
        outs.append(torch.lerp(b_, buf, cov.expand_as(buf)))
    return torch.cat(outs, -1)


LEAVES = ('col', 'wide', 's1', 's2', 's3', 's5', 'ones')


def _aa_inputs(name):
    posn, f, H, W, nb = case_scene(name)
    g = _gen(name, 'aa')
    r = lambda *s: torch.rand(*s, generator=g)
    n = lambda *s: torch.randn(*s, generator=g)
    inp = {'col': r(nb, H, W, 3), 'pw': _pixel_weight(name), 'wide': n(nb, H, W, 6), 's1': n(nb, H, W, 3), 's2': r(nb, H, W, 1) * 3, 's3': r(nb, H, W, 1) * 2 - 1, 's5': n(1, H, W, 2),
           'ones': torch.ones(nb, H, W, 1), 'bg': r(1 if posn.shape[0] == 1 else nb, H, W, 3), 'target': r(nb, H, W, 1) * 0.5,
           'G_sep': 0.5 + r(nb, H, W, 3), 'G_fused': 0.5 + r(nb, H, W, 18)}
    return inp


def foreground_colour(col, rast):
    """the random colour image made bright (0.6 .. 1) on the mesh and dark (0 .. 0.2) beside it, so that every blend along the silhouette moves
    the energy of the image the same way"""
    cov = rast[..., 3:] > 0
    return torch.where(cov, 0.6 + 0.4 * col, 0.2 * col)


def six_sources(t, bg):
    """the six source kinds of check_composite_antialias_fused: image background, zero, constant 20, alpha-only, a strided slice, a broadcast source"""
    return [(t['wide'][..., 0:3], COMP_IMAGE, bg), (t['s1'], COMP_ZERO, None), (t['s2'], COMP_CONST20, None), (t['s3'], COMP_ALPHA, None),
            (t['wide'][..., 3:6], COMP_ZERO, None), (t['s5'], COMP_ZERO, None)]


def _losses(out_sep, out_fused, out_mask, inp, keep, cast):
    """the three scalar losses; `keep` [B,H,W,1] zeroes the upstream gradient on the pixels of the pairs next to a kink.  Separate and fused:
    the weighted ENERGY sum(G pw out^2), G in 0.5 .. 1.5, pw = _pixel_weight: a blend moves a pixel towards its neighbour across the silhouette,
    and with a foreground brighter than the background (separate), a zero background (four of the six sources) or the constant 20 (one) each
    channel's energy changes with one sign under a dilation, so the dilation derivative and, through pw, the vertex sum are well conditioned.
    The mask chain: ((out - target)^2).sum(), the product's loss."""
    kw = keep * cast(inp['pw'])
    return ((out_sep ** 2 * cast(inp['G_sep']) * kw).sum(), (out_fused ** 2 * cast(inp['G_fused']) * kw).sum(),
            (keep * (out_mask - cast(inp['target'])) ** 2).sum())


def kink_keep(pb, pi, po, d, nb, npix):
    """-> (near [pairs] bool: d within KINK of 0.5, 0 or 1; keep [nb, npix] bool: False on both pixels of every such pair)"""
    near = ((d - 0.5).abs() < KINK) | (d < KINK) | (d > 1.0 - KINK)
    keep = torch.ones(nb, npix, dtype=torch.bool)
    keep[pb[near], pi[near]] = False
    keep[pb[near], po[near]] = False
    return near, keep


def check_kink_masking():
    """JITTER_SEED is the first seed at which no pair of any case is dropped (with 36 .. 90 pairs per case the 2 % cap allows none), so the
    cases themselves never run the masking: synthetic pairs do"""
    d = torch.tensor([0.25, 0.5 + 0.5 * KINK, 0.5 - 2 * KINK, 0.5 * KINK, 1.0 - 0.5 * KINK, 0.75, -1e-5, 0.5], dtype=torch.float64)
    pb = torch.tensor([0, 0, 0, 1, 1, 1, 0, 1])
    pi = torch.tensor([0, 2, 4, 6, 8, 10, 12, 14])
    po = pi + 1
    near, keep = kink_keep(pb, pi, po, d, 2, 16)
    assert near.tolist() == [False, True, False, True, True, False, True, True]
    dropped = {(0, 2), (0, 3), (1, 6), (1, 7), (1, 8), (1, 9), (0, 12), (0, 13), (1, 14), (1, 15)}
    assert {(b, p) for b in range(2) for p in range(16) if not keep[b, p]} == dropped
    # the losses see nothing of a dropped pixel: the gradient with respect to the image is zero exactly there
    out = torch.rand(2, 4, 4, 1, dtype=torch.float64).requires_grad_(True)
    inp = {'pw': torch.ones(2, 4, 4, 1), 'G_sep': torch.ones(2, 4, 4, 1), 'G_fused': torch.ones(2, 4, 4, 1), 'target': torch.zeros(2, 4, 4, 1)}
    for L in _losses(out, out, out, inp, keep.reshape(2, 4, 4, 1).double(), lambda x: x.double()):
        g, = torch.autograd.grad(L, out)
        assert ((g == 0).reshape(2, 16) == ~keep).all()
    # ... and the forward comparison leaves them out
    a, b = torch.zeros(2, 4, 4, 1), torch.ones(2, 4, 4, 1)
    a[keep.reshape(2, 4, 4, 1)] = 1.0
    assert _err(a, b, keep.reshape(2, 4, 4, 1).double()) == (0.0, 0.0) and _err(a, b)[0] > 0


def _aa_reference(name):
    if ('aa', name) in _REF:
        return _REF[('aa', name)]
    from oracle import raster as OR
    posn, f, H, W, nb = case_scene(name)
    inp = _aa_inputs(name)
    tri_o = torch.from_numpy(f)
    rast, _ = OR.rasterize(torch.from_numpy(posn).expand(nb, -1, -1), tri_o, H, W)
    rast = rast.detach()
    out = {'rast': rast}
    keep = None
    for dt in (torch.float64, torch.float32):              # (float64 first: its d decides which pairs are dropped, for every run)
        with _default_dtype(dt):
            t = {k: inp[k].to(dt).clone().requires_grad_(True) for k in LEAVES}
            pos = torch.from_numpy(posn).to(dt).requires_grad_(True)
            stack = torch.cat((foreground_colour(t['col'], rast), ref_composite(rast, six_sources(t, inp['bg'])), ref_composite(rast, [(t['ones'], COMP_ALPHA, None)])), -1)
            o, (pb, pi, po, d) = OR.antialias(stack, rast, pos, tri_o, return_pairs=True)
            if keep is None:
                near, keepf = kink_keep(pb, pi, po, d, nb, H * W)
                frac = float(near.double().mean())
                print(f'[raster64] ref  {name} {len(d)} pairs, {int(near.sum())} within {KINK} of a kink dropped ({100 * frac:.2f} %)')
                assert len(d) >= 25, len(d)
                assert frac <= MAX_DROPPED, (name, frac)
                keep = keepf.reshape(nb, H, W, 1)
                out['keep'], out['pairs'], out['dropped'] = keep, len(d), frac
            o_sep, o_fused, o_mask = o[..., :3], o[..., 3:21], o[..., 21:]
            L = _losses(o_sep, o_fused, o_mask, inp, keep.to(dt), lambda x: x.to(dt))
            g_sep = torch.autograd.grad(L[0], [t['col'], pos], retain_graph=True)
            g_fused = torch.autograd.grad(L[1], [t[k] for k in ('wide', 's1', 's2', 's3', 's5')] + [pos], retain_graph=True)
            g_mask = torch.autograd.grad(L[2], [t['ones'], pos])
        out[dt] = {'sep.out': o_sep.detach(), 'sep.d_color': g_sep[0], 'sep.d_pos': g_sep[1], 'fused.out': o_fused.detach(),
                   **{f'fused.d_{k}': g_ for k, g_ in zip(('wide', 's1', 's2', 's3', 's5'), g_fused[:5])}, 'fused.d_pos': g_fused[5],
                   'mask.out': o_mask.detach(), 'mask.d_src': g_mask[0], 'mask.d_pos': g_mask[1]}
    assert float((out[torch.float64]['sep.out'] - foreground_colour(inp['col'], rast).double()).abs().max()) > 1e-3          # something was blended
    _REF[('aa', name)] = out
    return out


def run_aa(dev, name):
    if 'sep.out' in RESULTS.get((dev, name), {'tensors': {}})['tensors']:
        return RESULTS[(dev, name)]
    from d3h import imgops as I, raster
    assert (I.COMP_ZERO, I.COMP_IMAGE, I.COMP_CONST20, I.COMP_ALPHA) == (COMP_ZERO, COMP_IMAGE, COMP_CONST20, COMP_ALPHA)
    posn, f, H, W, nb = case_scene(name)
    inp = _aa_inputs(name)
    ref = _aa_reference(name)
    r32, r64, keep = ref[torch.float32], ref[torch.float64], ref['keep']
    rast, tri = ref['rast'].to(dev).contiguous(), T(f.astype(np.int32), dev)
    keep_d, bg = keep.float().to(dev), inp['bg'].to(dev)
    cast = lambda x: x.to(dev)
    got = {}
    dpos = {}
    for fused in (True, False):
        t = {k: inp[k].clone().to(dev).requires_grad_(True) for k in LEAVES}
        pos = [T(posn, dev, True) for _ in range(3)]
        if fused:
            o_sep = raster.antialias(foreground_colour(t['col'], rast), rast, pos[0], tri)
            o_fused = I.composite_antialias_grad(rast, six_sources(t, bg), pos[1], tri)
            o_mask = I.composite_antialias_grad(rast, [(t['ones'], COMP_ALPHA, None)], pos[2], tri)
        else:
            o_sep = None
            o_fused = raster.antialias(I.composite(rast, six_sources(t, bg)), rast, pos[1], tri)
            o_mask = raster.antialias(I.composite(rast, [(t['ones'], COMP_ALPHA, None)]), rast, pos[2], tri)
        L = _losses(o_sep if fused else torch.zeros((), device=dev), o_fused, o_mask, inp, keep_d, cast)
        sum(L[0 if fused else 1:]).backward()
        dpos[fused] = (pos[1].grad, pos[2].grad)
        if fused:
            got = {'sep.out': o_sep, 'sep.d_color': t['col'].grad, 'sep.d_pos': pos[0].grad, 'fused.out': o_fused,
                   **{f'fused.d_{k}': t[k].grad for k in ('wide', 's1', 's2', 's3', 's5')}, 'fused.d_pos': pos[1].grad,
                   'mask.out': o_mask, 'mask.d_src': t['ones'].grad, 'mask.d_pos': pos[2].grad}
        else:
            # one kernel each way against the two separate ops: values bit for bit, d_pos up to the order of its float atomics
            assert torch.equal(o_fused.detach(), got['fused.out'].detach()) and torch.equal(o_mask.detach(), got['mask.out'].detach())
            for k in (0, 1):
                assert float(dpos[False][k].abs().max()) > 0
                assert (dpos[True][k] - dpos[False][k]).abs().max() <= 1e-5 * dpos[False][k].abs().max(), (name, k)
    kd = keep.double()
    for k in got:
        is_out = k.endswith('.out')
        _record(dev, name, k, got[k], r32[k], r64[k], keep=kd if is_out else None, posn=posn if k.endswith('d_pos') else None)
    res = RESULTS[(dev, name)]
    res['pairs'], res['dropped'] = ref['pairs'], ref['dropped']
    return res


# ---- the bar ----------------------------------------------------------------------------------------------------------------------------------
def _rms(xs):
    return float(np.sqrt(np.mean(np.square(xs))))


def check_bar(dev, names, label):
    """over `names`: RMS(e_k) <= 3 RMS(e_32) per tensor (relative L2), and the same for the dilation derivative and the vertex sum of every
    d_pos (module docstring)"""
    rows = []
    for n in names:
        run_raster(dev, n)
        rows.append(run_aa(dev, n))
    bad = []
    for tname in rows[0]['tensors']:
        ek, e32 = _rms([r['tensors'][tname][0] for r in rows]), _rms([r['tensors'][tname][1] for r in rows])
        mk, m32 = _rms([r['tensors'][tname][2] for r in rows]), _rms([r['tensors'][tname][3] for r in rows])
        print(f'[raster64] {dev:4s} {label} RMS {tname:22s} L2 kernel {ek:.3e} oracle32 {e32:.3e} ratio {ek / e32 if e32 else float(ek > 0):.2f} | '
              f'max kernel {mk:.3e} oracle32 {m32:.3e}')
        if not ek <= RATIO * e32:
            bad.append((tname, 'L2', ek, e32))
    for tname in rows[0]['sums']:
        for col, what in ((0, 'dilation'), (2, 'vertex sum')):
            sk, s32 = _rms([r['sums'][tname][col] for r in rows]), _rms([r['sums'][tname][col + 1] for r in rows])
            print(f'[raster64] {dev:4s} {label} RMS {tname:22s} {what:10s} kernel {sk:.3e} oracle32 {s32:.3e} ratio {sk / s32 if s32 else float(sk > 0):.2f}')
            if not sk <= RATIO * s32:
                bad.append((tname, what, sk, s32))
    assert not bad, bad


# ---- edges of the antialias kernels, against the float32 oracle with the bars of check_antialias ------------------------------------------------
AA_SHAPES = [(37, 53, 1), (37, 53, 3), (41, 29, 5), (33, 65, 9), (40, 40, 2)]
# sources whose composited channel total equals C (1, 3, 5, 9, 2: none a multiple of 4): (channels, kind)
AA_FUSED_SOURCES = {1: [(1, COMP_ALPHA)], 3: [(2, COMP_ZERO)], 5: [(3, COMP_IMAGE), (1, COMP_ALPHA)], 9: [(3, COMP_ZERO), (1, COMP_CONST20), (2, COMP_ZERO)],
                    2: [(1, COMP_CONST20)]}


def _aa_against_oracle(dev, posn, f, H, W, C, specs, gen):
    """separate antialias on a random C-channel image and the fused pair on `specs`, both against oracle/raster.py in float32: values 1e-4,
    colour / source gradients 1e-4, d_pos 2e-3 of its largest entry (check_antialias); fused == separate as check_composite_antialias_fused.
    -> (colour, kernel output, oracle output, upstream gradient, kernel d_color) of the separate run"""
    from d3h import imgops as I, raster
    from oracle import raster as OR
    nb = 2 if posn.shape[0] == 1 else posn.shape[0]
    tri_o, tri = torch.from_numpy(f), T(f.astype(np.int32), dev)
    rast_o, _ = OR.rasterize(torch.from_numpy(posn).expand(nb, -1, -1), tri_o, H, W)
    rast = rast_o.to(dev).contiguous()
    coln = torch.rand(nb, H, W, C, generator=gen)
    col, col_o = coln.clone().to(dev).requires_grad_(True), coln.clone().requires_grad_(True)
    pos, pos_o = T(posn, dev, True), torch.from_numpy(posn).requires_grad_(True)
    out = raster.antialias(col, rast, pos, tri)
    out_o = OR.antialias(col_o, rast_o, pos_o, tri_o)
    assert (out_o.detach() - coln).abs().max() > 1e-3
    assert (out.detach().cpu() - out_o.detach()).abs().max() < 1e-4
    G = torch.randn(out_o.shape, generator=gen)
    (out * G.to(dev)).sum().backward()
    (out_o * G).sum().backward()
    assert (col.grad.cpu() - col_o.grad).abs().max() < 1e-4
    assert pos_o.grad.abs().max() > 0
    assert (pos.grad.cpu() - pos_o.grad).abs().max() < 2e-3 * pos_o.grad.abs().max()
    # the fused pair
    srcn = [(torch.randn(nb, H, W, c, generator=gen) if k != COMP_ALPHA else torch.rand(nb, H, W, c, generator=gen), k,
             torch.rand(nb, H, W, 3, generator=gen) if k == COMP_IMAGE else None) for c, k in specs]
    Gf = torch.randn(nb, H, W, sum(1 if k == COMP_ALPHA else c + 1 for c, k in specs), generator=gen)
    leaf_o = [s.clone().requires_grad_(True) for s, _, _ in srcn]
    pos_o = torch.from_numpy(posn).requires_grad_(True)
    of_o = OR.antialias(ref_composite(rast_o, [(t, k, b) for t, (_, k, b) in zip(leaf_o, srcn)]), rast_o, pos_o, tri_o)
    assert of_o.shape == Gf.shape
    (of_o * Gf).sum().backward()
    res = []
    for fused in (True, False):
        leaf = [s.clone().to(dev).requires_grad_(True) for s, _, _ in srcn]
        srcs = [(t, k, None if b is None else b.to(dev)) for t, (_, k, b) in zip(leaf, srcn)]
        p = T(posn, dev, True)
        if fused:
            with torch.no_grad():
                fwd_only = I.composite_antialias(rast, [(t.detach(), k, b) for t, k, b in srcs], p.detach(), tri)
            of = I.composite_antialias_grad(rast, srcs, p, tri)
            assert torch.equal(fwd_only, of.detach())
        else:
            of = raster.antialias(I.composite(rast, srcs), rast, p, tri)
        (of * Gf.to(dev)).sum().backward()
        res.append((of.detach(), [t.grad for t in leaf], p.grad))
        assert (of.detach().cpu() - of_o.detach()).abs().max() < 1e-4
        for t, t_o in zip(leaf, leaf_o):
            assert (t.grad.cpu() - t_o.grad).abs().max() < 1e-4
        assert (p.grad.cpu() - pos_o.grad).abs().max() < 2e-3 * pos_o.grad.abs().max()
    assert torch.equal(res[0][0], res[1][0])
    assert all(torch.equal(a, b) for a, b in zip(res[0][1], res[1][1]))
    assert (res[0][2] - res[1][2]).abs().max() <= 1e-5 * res[1][2].abs().max()
    return coln, out.detach().cpu(), out_o.detach(), G, col.grad.cpu()


def check_aa_copy_branch(dev, shape):
    """frame sizes whose last workgroup holds a float count that is no multiple of 4: the scalar copy branch of aa_fwd_kernel / aa_bwd_kernel (the
    `else` of (cnt & 3) == 0 && ((p0 * C) & 3) == 0), and the same shapes through the fused kernels with a channel total that is no multiple of 4"""
    H, W, C = shape
    posn, f = _raster_scene(40, 2)
    _aa_against_oracle(dev, posn, f, H, W, C, AA_FUSED_SOURCES[C], torch.Generator().manual_seed(100 + C))


def check_aa_shapes_reach_the_scalar_branch():
    odd = [s for s in AA_SHAPES if (((2 * s[0] * s[1]) % 512) * s[2]) % 4 != 0]
    assert len(odd) >= 3, odd


def check_aa_three_routes_agree_bit_for_bit(dev):
    """EMULATION ONLY (it runs the blocks serially, so the float atomics of d_pos come in one order; on the GPU they do not).  The same
    pre-antialias image by the three pairs of kernels: antialias(composite(...)), composite_antialias_grad, and layer_composite_antialias with
    alpha=None over under = zeros.  Two COMP_ZERO sources of 3 and 2 channels: composite writes [src, 1] where covered and 0 elsewhere, the
    layer's two-branch lerp is exact at weight 1 (covered) and 0 (not), so all three see the same image and share every later operation:
    outputs and d_pos are equal bit for bit.  Nothing else ties the layer kernel's position gradient to the other two."""
    from d3h import imgops as I, raster
    from oracle import raster as OR
    H = W = 40
    posn, f = _raster_scene(40, 2)
    tri_o, tri = torch.from_numpy(f), T(f.astype(np.int32), dev)
    rast_o, _ = OR.rasterize(torch.from_numpy(posn), tri_o, H, W)
    rast = rast_o.to(dev).contiguous()
    gen = torch.Generator().manual_seed(77)
    srcn = [torch.randn(2, H, W, 3, generator=gen), torch.randn(2, H, W, 2, generator=gen)]
    G = torch.randn(2, H, W, 7, generator=gen).to(dev)
    outs, dpos = [], []
    for route in range(3):
        srcs = [(s.clone().to(dev).requires_grad_(True), COMP_ZERO, None) for s in srcn]
        pos = T(posn, dev, True)
        if route == 0:
            out = raster.antialias(I.composite(rast, srcs), rast, pos, tri)
        elif route == 1:
            out = I.composite_antialias_grad(rast, srcs, pos, tri)
        else:
            out = I.layer_composite_antialias(rast, srcs, None, torch.zeros(2, H, W, 7, device=dev), pos, tri)
        (out * G).sum().backward()
        outs.append(out.detach())
        dpos.append(pos.grad)
    nz = int((dpos[0] != 0).sum())
    print(f'[raster64] {dev:4s} three routes: {nz} non-zero d_pos entries')
    assert tuple(outs[0].shape) == (2, H, W, 7) and nz > 0
    for k in (1, 2):
        assert torch.equal(outs[k], outs[0]), k
        assert torch.equal(dpos[k], dpos[0]), k


def _quad(px, H, W, z=0.1):
    """four pixel-space corners -> clip positions [4, 4] with w = 1"""
    return np.array([[x / W * 2 - 1, y / H * 2 - 1, z, 1.0] for x, y in px], np.float32)


QUAD_FACES = np.array([[0, 1, 2], [0, 2, 3]], np.int64)


def check_aa_wave_boundary(dev):
    """a near-vertical silhouette between the pixel columns 63 | 64 of a 32 x 160 frame: on the even rows the flat indices of the two pixels are
    64 k - 1 | 64 k, the last lane of one wave and the first of the next (the lane-0 / lane-63 reload of aa_on_discontinuity); the edge runs from
    x = 63.8 to x = 64.3, so the blended pixel is in column 63 on the upper rows (d < 0.5) and in column 64 on the lower ones"""
    H, W = 32, 160
    posn = _quad([(20.3, 3.3), (63.8, 3.3), (64.3, 28.6), (20.3, 28.6)], H, W)[None]
    col, out, out_o, _, _ = _aa_against_oracle(dev, posn, QUAD_FACES, H, W, 3, [(3, COMP_ZERO)], torch.Generator().manual_seed(31))
    even = torch.arange(4, 28, 2)
    assert ((W * even + 63) % 64 == 63).all()
    for o in (out_o, out):
        changed = (o != col).any(-1)
        assert changed[:, even, 63].any() and changed[:, even, 64].any()
        assert not changed[:, 5:27, 62].any() and not changed[:, :, 65].any()


def check_aa_frame_boundary(dev):
    """two frames; the last row of frame 0 is covered, with the silhouette running just below it (y = 23.8 .. 24.3 of 24 rows), the first row of
    frame 1 is empty.  Rows of consecutive frames are consecutive in memory: a pair formed across the frame boundary would blend the last row
    of frame 0 with the first of frame 1.  Nothing may: away from the quad's side edges both rows come out as they went in, values and gradient."""
    H, W = 24, 40
    p0 = _quad([(5.3, 10.4), (33.6, 10.4), (33.6, 24.3), (5.3, 23.8)], H, W)
    p1 = _quad([(5.3, 6.4), (33.6, 6.4), (33.6, 20.3), (5.3, 19.8)], H, W)
    posn = np.stack([p0, p1])
    col, out, out_o, G, d_col = _aa_against_oracle(dev, posn, QUAD_FACES, H, W, 3, [(3, COMP_ZERO)], torch.Generator().manual_seed(32))
    from oracle import raster as OR
    ids = OR.rasterize_ids(posn, QUAD_FACES, H, W)
    assert (ids[0, H - 1, 6:33] > 0).all() and (ids[1, 0] == 0).all()
    for o in (out_o, out):
        assert torch.equal(o[0, H - 1, 7:32], col[0, H - 1, 7:32]) and torch.equal(o[1, 0], col[1, 0])
    assert torch.equal(d_col[0, H - 1, 7:32], G[0, H - 1, 7:32]) and torch.equal(d_col[1, 0], G[1, 0])
