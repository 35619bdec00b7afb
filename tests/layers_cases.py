"""Check functions of layered rendering -- depth-peeled layers shaded one by one and blended back to front, the opacity in the fourth channel of kd
(render.render.render_mesh(num_layers=..., FLAGS.transparency), d3h.imgops.layer_composite_antialias, csrc/raster.hip: layer_composite_*_kernel,
d3h.export.textured_mesh(transparency=True)) -- shared by tests/test_layers_emul.py (host emulation of the kernel sources) and tests/test_gpu_layers.py
(MI355X).  Same shapes on both: two concentric synth.icosphere(1) shells of radius 0.6 and 0.35 in one mesh (depth complexity 4 along central rays),
B = 2 frames of 37 x 53 pixels (no multiple of 256 or of the 512-pixel workgroup tile, more than one workgroup), maps of 64 x 64, a smooth opacity in
[0.2, 0.9].

Yardstick: `y_render` / `y_step` below, the contract of render/render.py's docstring restated in dtype-generic torch -- per layer the lookups and the
shading of tests/texmat_cases.py (y_*), torch.lerp, and oracle.raster.antialias on the channel-concatenated image -- evaluated in float64 and in
float32 on the CPU from the float32 run's OWN rasters (the visibility decisions are shared).  Parity rule (tests/uvatlas_cases.py:assert_close):
max|got - f64| / max|f64| <= max(5 * the float32 yardstick's own distance from float64, 2^-20).  Every figure is printed before it is asserted (-s).

Input condition, asserted when the scene is built: no blended pixel pair of any layer sits within 1e-4 of the kink of |d - 0.5| in the float32 run."""
import ctypes
import functools
import os

import pytest
import torch

import texmat_cases as TC
from texmat_cases import B, H, W, TEX
from uvatlas_cases import FLOOR, _PositionAsColour, assert_close, assert_floor, rel

LAYERS = 4
RADII = (0.6, 0.35)


def _cpu(t):
    return t.detach().cpu()


# ---- the scene -------------------------------------------------------------------------------------------------------------------------------
def _alpha_map(res):
    """smooth, non-constant, within [0.2, 0.9]"""
    y, x = torch.meshgrid(torch.arange(res, dtype=torch.float32) / res, torch.arange(res, dtype=torch.float32) / res, indexing='ij')
    a = 0.55 + 0.35 * torch.sin(7.0 * x + 1.0) * torch.cos(5.0 * y)
    assert 0.2 <= float(a.min()) < 0.3 and 0.8 < float(a.max()) <= 0.9
    return a


def scene(dev, alpha=None):
    """-> (exported two-shell mesh with tangents and a 4-channel kd, mvp, campos, draws); alpha: None = the smooth map, or a number"""
    import numpy as np
    from d3h import export, synth
    from render import mesh as rmesh
    v, t = synth.icosphere(1)
    v, t = np.asarray(v, np.float32), np.asarray(t, np.int64)
    # turned out of its axis-aligned pose: the icosphere has edges in the plane y = 0, which the middle row of pixel centres of an odd-height frame
    # lies in exactly -- both triangles of such an edge cover those centres at equal depth and the peeler reports each (d3h/raster.py: ties), eight
    # layers along that row where the test wants four
    cx, sx, cz, sz = np.cos(0.3), np.sin(0.3), np.cos(0.2), np.sin(0.2)
    v = (v @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]).T @ np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]).T).astype(np.float32)
    vv = np.concatenate([v * np.float32(r) for r in RADII]).astype(np.float32)
    tt = np.concatenate([t + k * len(v) for k in range(len(RADII))])
    _, _, mvp, cam, draws = TC._scene_np()
    mat = {'bsdf': 'pbr', 'kd_ks': _PositionAsColour()}
    base = rmesh.auto_normals(rmesh.Mesh(TC._t(vv, dev), TC._t(tt, dev), material=mat))
    ex = export.textured_mesh(base, mat, TEX, [-1.0] * 3, [1.0] * 3, [-1.0] * 3, [1.0] * 3, [-1.0, -1.0, 0.0], [1.0, 1.0, 1.0], transparency=True)
    ex = rmesh.compute_tangents(ex)
    kd = ex.material['kd']
    assert tuple(kd.data.shape) == (1, TEX, TEX, 4) and kd.data.requires_grad and bool((kd.data[..., 3] == 1).all())
    assert [float(x) for x in kd.min_max[0]] == [-1.0, -1.0, -1.0, 0.0] and [float(x) for x in kd.min_max[1]] == [1.0] * 4
    with torch.no_grad():
        kd.data[..., 3] = _alpha_map(TEX).to(dev) if alpha is None else float(alpha)
        ex.material['normal'].data.copy_(TC._t(TC.TILT, dev, torch.float32).expand_as(ex.material['normal'].data))
    return ex, mvp.to(dev), cam.to(dev), draws


class _Flags:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def render(mesh, mvp, cam, draws, layers=LAYERS, transparency=True, fused=None, flags=None, **kw):
    """render_mesh under fixed draws; fused None: the default route, True / False: D3H_LAYER_FUSED forced"""
    import nvdiffrast.torch as dr
    from render import render as rr
    old = os.environ.get('D3H_LAYER_FUSED')
    if fused is not None:
        os.environ['D3H_LAYER_FUSED'] = '1' if fused else '0'
    try:
        fl = flags if flags is not None else (_Flags(transparency=True) if transparency else _Flags())
        return rr.render_mesh(fl, 0, dr.RasterizeGLContext(), mesh, None, mvp, cam, None, [H, W], num_layers=layers, _rng_draws=draws, **kw)
    finally:
        if fused is not None:
            if old is None:
                del os.environ['D3H_LAYER_FUSED']
            else:
                os.environ['D3H_LAYER_FUSED'] = old


def routes_taken(fn):
    """run fn() and count the blend steps per route: {'fused': n, 'composed': n}"""
    from d3h import imgops
    n = {'fused': 0, 'composed': 0}
    f0, l0 = imgops.layer_composite_antialias, torch.lerp

    def f1(*a, **k):
        n['fused'] += 1
        return f0(*a, **k)

    def l1(*a, **k):
        n['composed'] += 1
        return l0(*a, **k)
    imgops.layer_composite_antialias, torch.lerp = f1, l1
    try:
        out = fn()
    finally:
        imgops.layer_composite_antialias, torch.lerp = f0, l0
    return out, n


_STATE = {}


def state(dev):
    """the scene, its peeled rasters (the float32 run's own: the decisions every yardstick shares) and the input condition; built once per device"""
    if dev in _STATE:
        return _STATE[dev]
    import nvdiffrast.torch as dr
    from oracle import raster as OR
    from render import renderutils as ru
    ex, mvp, cam, draws = scene(dev)
    with torch.no_grad():
        clip = ru.xfm_points(ex.v_pos[None], mvp)
        with dr.DepthPeeler(dr.RasterizeGLContext(), clip, ex.t_pos_idx32, [H, W], grad_db=False) as peeler:
            peeled = [peeler.rasterize_next_layer(want_db=True) for _ in range(LAYERS + 1)]
    rasts, dbs = [_cpu(r) for r, _ in peeled], [_cpu(d) for _, d in peeled]
    assert not rasts[LAYERS].any(), 'the scene has more than four layers'
    covered = [int((r[..., 3] > 0).sum()) for r in rasts[:LAYERS]]
    print('covered pixels per layer:', covered)
    assert all(c > 100 for c in covered) and covered[0] >= covered[1] > covered[2] >= covered[3]
    E = TC._ex_np(ex)
    # input condition: the kink of the blend weight |d - 0.5|
    worst, pairs = 1.0, []
    for r in rasts[:LAYERS]:
        _, (_, _, _, d) = OR.antialias(torch.zeros(B, H, W, 1), r, _cpu(clip), E['tri'], return_pairs=True)
        pairs.append(d.numel())
        worst = min([worst] + (d - 0.5).abs().tolist())
    print('blended pairs per layer:', pairs)             # (the deepest layer ends where the inner shell does: no silhouette of its own triangles)
    assert min(pairs[:3]) > 20
    print(f'closest blended pair to the kink of |d - 0.5|: {worst:.3e}')
    assert worst >= 1e-4
    S = {'ex': ex, 'mvp': mvp, 'cam': cam, 'draws': draws, 'rasts': rasts[:LAYERS], 'dbs': dbs[:LAYERS], 'E': E, 'clip': _cpu(clip)}
    g = torch.Generator().manual_seed(71)
    S['msdf'] = torch.rand(ex.v_pos.shape[0], generator=g) * 0.8 + 0.1
    _STATE[dev] = S
    return S


# ---- the yardstick -----------------------------------------------------------------------------------------------------------------------------
def y_step(under, ends, weights, rast, clip, tri):
    """one step of the contract: antialias(lerp(under, end_k, w_k) per buffer k, rast, clip, tri) on lists of [B,H,W,n_k + 1] images"""
    from oracle import raster as OR
    pre = torch.cat([torch.lerp(u, e, w) for u, e, w in zip(under, ends, weights)], dim=-1)
    out = OR.antialias(pre, rast, clip, tri)
    return list(torch.split(out, [u.shape[-1] for u in under], dim=-1))


def y_clip(p, mvp, dtype):
    return torch.matmul(torch.nn.functional.pad(p, (0, 1), value=1.0)[None], mvp.cpu().to(dtype).transpose(1, 2))


def y_render(S, dtype, keys, maps=None, v_pos=None, background=None, layers=LAYERS):
    """section 1 of the contract in `dtype`: {buffer: [B,H,W,n + 1]} (msdf_image: one channel).  maps: (kd [1,h,w,4], ks, normal) in `dtype` (None:
    the scene's); v_pos given (a differentiable [V,3]): barycentrics, clip positions and interpolated positions are functions of it"""
    from oracle import raster as OR
    E, draws, cam = S['E'], S['draws'], S['cam'].cpu()
    tri, tex_idx = E['tri'], E['t_tex_idx']
    if maps is None:
        maps = [_cpu(S['ex'].material[k].data).to(dtype) for k in ('kd', 'ks', 'normal')]
    kd4, ks, nrm = maps
    p = E['v_pos'].to(dtype) if v_pos is None else v_pos
    clip = y_clip(p, S['mvp'], dtype)
    view = cam.to(dtype)[:, None, None, :]
    one = torch.ones(B, H, W, 1, dtype=dtype)
    acc = {}
    for k in keys:
        if k == 'msdf_image':
            acc[k] = torch.zeros(B, H, W, 1, dtype=dtype)
        elif k == 'shaded':
            bg = torch.zeros(1, H, W, 3) if background is None else background.cpu()
            acc[k] = torch.cat((bg.to(dtype).expand(B, H, W, 3), torch.zeros(B, H, W, 1, dtype=dtype)), dim=-1)
        elif k == 'depth':
            acc[k] = torch.full((B, H, W, 2), 20.0, dtype=dtype)
        else:
            acc[k] = torch.zeros(B, H, W, 2 if k == 'invdepth' else 4, dtype=dtype)
    for l in reversed(range(min(layers, LAYERS))):
        rast, db = S['rasts'][l], S['dbs'][l]
        yb = TC._y_buffers(E, rast, clip if v_pos is not None else None, [kd4[..., :3], ks], nrm, draws, cam, dtype, v_pos=v_pos)
        r = rast.to(dtype)
        if v_pos is not None:
            r = torch.cat((TC.y_rast_uv(clip, tri, rast), r[..., 2:]), -1)
        cov = (rast[..., 3:4] > 0).to(dtype)
        alpha = TC.y_bilinear(kd4[..., 3:4], TC.y_interp(E['v_tex'].to(dtype), r, tex_idx), 'wrap') * cov
        gb_pos = TC.y_interp(p, r, tri)
        if 'geometric_normal' in keys:
            fn = TC.y_normalize(torch.cross(p[tri[:, 1]] - p[tri[:, 0]], p[tri[:, 2]] - p[tri[:, 0]], dim=-1))
            ids = rast[..., 3].long()
            yb['geometric_normal'] = torch.where((ids > 0)[..., None], fn[(ids - 1).clamp(min=0)], torch.zeros_like(gb_pos))
        d = gb_pos - view
        yb['depth'] = d.pow(2).sum(dim=-1, keepdim=True).sqrt()
        yb['invdepth'] = 1.0 / (d.pow(2) + 1e-8).sum(dim=-1, keepdim=True).sqrt()
        if 'z_grad' in keys:
            eps = 0.00001
            cp, cpd = OR.interpolate(clip.detach(), r.detach(), tri, rast_db=db.to(dtype))
            z0 = torch.clamp(cp[..., 2:3], min=eps) / torch.clamp(cp[..., 3:4], min=eps)
            z1 = torch.clamp(cp[..., 2:3] + torch.abs(cpd[..., 2:3]), min=eps) / torch.clamp(cp[..., 3:4] + torch.abs(cpd[..., 3:4]), min=eps)
            yb['z_grad'] = torch.cat((z0, torch.abs(z1 - z0), torch.zeros_like(z0)), dim=-1)
        w = cov * alpha
        ends, weights = [], []
        for k in keys:
            if k == 'msdf_image':
                ends.append(one)
                weights.append(cov * TC.y_interp(S['msdf'].to(dtype)[:, None], r, tri))
            else:
                ends.append(torch.cat((yb[k], one), dim=-1))
                weights.append(w)
        acc = dict(zip(keys, y_step([acc[k] for k in keys], ends, weights, rast, clip, tri)))
    return acc


_Y = {}


def yard(S, keys, background=None):
    """(float64, float32) restatements of the scene as it stands, computed once per key set and shared"""
    key = (id(S), tuple(keys), None if background is None else float(background.reshape(-1)[0]))
    if key not in _Y:
        with torch.no_grad():
            _Y[key] = tuple(y_render(S, dt, keys, background=background) for dt in (torch.float64, torch.float32))
    return _Y[key]


def _public(out):
    return sorted(k for k in out if not k.startswith('_') and k != 'visible_triangles')


# ---- 1. the kernel alone -----------------------------------------------------------------------------------------------------------------------
KINDS = (0, 1, 2, 3)                    # COMP_ZERO, COMP_IMAGE, COMP_CONST20, COMP_ALPHA
WIDTHS = (3, 3, 1, 1)


@functools.lru_cache(maxsize=None)
def _kernel_inputs():
    g = torch.Generator().manual_seed(23)
    wide = torch.rand(B, H, W, 6, generator=g)                      # source 0 is a strided slice of it
    srcs = [wide[..., 1:4]] + [torch.rand(B, H, W, c, generator=g) for c in WIDTHS[1:]]
    alpha = torch.rand(B, H, W, 1, generator=g) * 0.8 + 0.1
    C = sum(1 if k == 3 else c + 1 for k, c in zip(KINDS, WIDTHS))
    under = torch.rand(B, H, W, C, generator=g) * 2.0 - 0.5
    wgt = torch.rand(B, H, W, C, generator=g, dtype=torch.float64) + 0.5
    return wide, srcs, alpha, under, wgt


def _y_kernel(S, layer, dtype, use_alpha=True):
    """-> (out, gradients of sum(out * wgt) to (wide, src1, src2, src3, alpha, under, clip))"""
    wide, srcs, alpha, under, wgt = _kernel_inputs()
    rast = S['rasts'][layer]
    leaf = lambda x: x.detach().to(dtype).clone().requires_grad_(True)
    leaves = [leaf(wide)] + [leaf(s) for s in srcs[1:]]
    a, u, clip = leaf(alpha), leaf(under), leaf(S['clip'])
    vals = [leaves[0][..., 1:4]] + leaves[1:]
    cov = (rast[..., 3:4] > 0).to(dtype)
    one = torch.ones(B, H, W, 1, dtype=dtype)
    w = cov * a if use_alpha else cov
    ends = [one if k == 3 else torch.cat((v, one), dim=-1) for k, v in zip(KINDS, vals)]
    weights = [cov * v if k == 3 else w for k, v in zip(KINDS, vals)]
    split = [1 if k == 3 else c + 1 for k, c in zip(KINDS, WIDTHS)]
    out = torch.cat(y_step(list(torch.split(u, split, dim=-1)), ends, weights, rast, clip, S['E']['tri']), dim=-1)
    (out * wgt.to(dtype)).sum().backward()
    return out.detach(), [x.grad for x in leaves] + [a.grad, u.grad, clip.grad]


def check_kernel(dev, layer, use_alpha=True):
    """layer_composite_antialias on a real peeled layer with random sources of all four kinds: values and every gradient"""
    from d3h import imgops as I
    S = state(dev)
    wide, srcs, alpha, under, wgt = _kernel_inputs()
    d = lambda x: x.to(dev)
    leaves = [d(wide).clone().requires_grad_(True)] + [d(s).clone().requires_grad_(True) for s in srcs[1:]]
    a, u = d(alpha).clone().requires_grad_(True), d(under).clone().requires_grad_(True)
    clip = S['clip'].to(dev).clone().requires_grad_(True)
    vals = [leaves[0][..., 1:4]] + leaves[1:]
    before = u.detach().clone()
    out = I.layer_composite_antialias(d(S['rasts'][layer]), list(zip(vals, KINDS)), a if use_alpha else None, u, clip, S['ex'].t_pos_idx32)
    assert tuple(out.shape) == tuple(under.shape) and torch.equal(u.detach(), before)
    (out * d(wgt).float()).sum().backward()
    y64, g64 = _y_kernel(S, layer, torch.float64, use_alpha)
    y32, g32 = _y_kernel(S, layer, torch.float32, use_alpha)
    what = f'layer {layer}' + ('' if use_alpha else ', alpha=None')
    assert_close(f'step values, {what}', out, y64, y32)
    got = [x.grad for x in leaves] + [a.grad, u.grad, clip.grad]
    names = ['source 0 (slice of a wider tensor)', 'source 1', 'source 2', 'source 3 (alpha-only)', 'alpha', 'under', 'pos']
    for n, gg, r64, r32 in zip(names, got, g64, g32):
        if n == 'alpha' and not use_alpha:
            assert gg is None
            continue
        assert gg is not None and float(r64.abs().max()) > 0, n
        assert_close(f'd / d {n}, {what}', gg, r64, r32)
    assert not got[0][..., 0].any() and not got[0][..., 4:].any()       # the channels of the wide tensor outside the slice
    with torch.no_grad():                                                # forward only: the same values
        again = I.layer_composite_antialias(d(S['rasts'][layer]), list(zip([v.detach() for v in vals], KINDS)), a.detach() if use_alpha else None,
                                            u.detach(), clip.detach(), S['ex'].t_pos_idx32)
    assert torch.equal(again, out.detach()) and not again.requires_grad


def _raw(dev, S, layer):
    """arguments of the two entry points for the kernel inputs on a peeled layer"""
    from d3h import _lib as L, raster as R
    wide, srcs, alpha, under, wgt = _kernel_inputs()
    d = lambda x: x.to(dev).contiguous()
    t = {'src': [d(s) for s in srcs], 'alpha': d(alpha), 'under': d(under), 'rast': d(S['rasts'][layer]), 'pos': d(S['clip']),
         'tri': S['ex'].t_pos_idx32.contiguous(), 'g': d(wgt).float()}
    t['flags'] = R._edge_flags(t['pos'], t['tri'], B, H, W)
    I4 = ctypes.c_int * 4
    t['tab'] = (I4(*WIDTHS), I4(*WIDTHS), I4(*KINDS))                  # stride, nch, kind (contiguous sources: stride = nch)
    return t, L, R


def _bwd_raw(L, R, t, ds, d_alpha, d_under, d_pos, alpha=True):
    stride, nch, kind = t['tab']
    L.call('layer_composite_antialias_bwd', 4, L.ptr_array(t['src']), L.ptr_array(ds), nch, stride, nch, kind, t['alpha'] if alpha else None, t['under'],
           t['rast'], t['pos'], R._bstride(t['pos']), t['tri'], t['tri'].shape[0], t['flags'], B, H, W, t['g'], d_alpha, d_under, d_pos)


def check_null_gradient_outputs(dev):
    """every subset of the gradient outputs: what is asked for is written completely (poisoned beforehand) with the same bits as when everything is
    asked for, what is not asked for does not exist; d_pos is accumulated"""
    S = state(dev)
    t, L, R = _raw(dev, S, 1)
    nan = lambda *s: torch.full(s, float('nan'), device=dev)
    full = {'ds': [nan(B, H, W, c) for c in WIDTHS], 'a': nan(B, H, W, 1), 'u': nan(*t['under'].shape), 'p': torch.zeros_like(t['pos'])}
    _bwd_raw(L, R, t, full['ds'], full['a'], full['u'], full['p'])
    for x in full['ds'] + [full['a'], full['u']]:
        assert bool(torch.isfinite(x).all()), 'a gradient output was not written completely'
    assert float(full['p'].abs().max()) > 0
    for keep in ((0,), (3,), (1, 2), ()):
        for want_a, want_u, want_p in ((False, False, False), (True, False, True), (False, True, False)):
            ds = [nan(B, H, W, c) if k in keep else None for k, c in enumerate(WIDTHS)]
            da, du = nan(B, H, W, 1) if want_a else None, nan(*t['under'].shape) if want_u else None
            dp = torch.ones_like(t['pos']) if want_p else None
            _bwd_raw(L, R, t, ds, da, du, dp)
            for k in keep:
                assert torch.equal(ds[k], full['ds'][k]), (keep, k)
            assert da is None or torch.equal(da, full['a'])
            assert du is None or torch.equal(du, full['u'])
            if dp is not None:                                         # accumulated onto the ones; float atomics reorder on the GPU
                assert_floor('d_pos accumulated', dp - 1.0, full['p'])
    if dev != 'cpu':
        torch.cuda.synchronize()


def check_channel_limit(dev):
    """the wrapper refuses more channels than the kernels have room for, before any call"""
    from d3h import imgops as I
    S = state(dev)
    rast, clip, tri = S['rasts'][0].to(dev), S['clip'].to(dev), S['ex'].t_pos_idx32
    src = torch.zeros(B, H, W, 5, device=dev)
    with pytest.raises(ValueError, match='channels'):
        I.layer_composite_antialias(rast, [(src, 0)] * 12, None, torch.zeros(B, H, W, 72, device=dev), clip, tri)
    s62 = [(src[..., :4], 0)] * 10 + [(src, 0)] * 2                     # 10 x 5 + 2 x 6 = 62 channels
    leaf = src[..., :4].clone().requires_grad_(True)
    with pytest.raises(ValueError, match='source gradient'):
        I.layer_composite_antialias(rast, [(leaf, 0)] + s62[1:], None, torch.zeros(B, H, W, 62, device=dev), clip, tri)
    out = I.layer_composite_antialias(rast, s62, None, torch.zeros(B, H, W, 62, device=dev), clip, tri)
    assert tuple(out.shape) == (B, H, W, 62)


def check_nothing_covered(dev):
    """a frame without a covered pixel, and a mesh without triangles: the step is the identity, bit for bit; d(under) = g, d(source) = 0"""
    from d3h import imgops as I
    S = state(dev)
    wide, srcs, alpha, under, wgt = _kernel_inputs()
    d = lambda x: x.to(dev)
    rast = S['rasts'][0].clone()
    rast[1] = 0
    cases = (('frame 1 empty', rast, S['ex'].t_pos_idx32, S['clip'].to(dev)),
             ('nf = 0', torch.zeros(B, H, W, 4), torch.zeros(0, 3, dtype=torch.int32, device=dev), S['clip'].to(dev)))
    for what, r, tri, clip in cases:
        leaves = [d(s).clone().requires_grad_(True) for s in srcs]
        a, u, p = d(alpha).clone().requires_grad_(True), d(under).clone().requires_grad_(True), clip.clone().requires_grad_(True)
        out = I.layer_composite_antialias(d(r), list(zip(leaves, KINDS)), a, u, p, tri)
        frames = (1,) if what == 'frame 1 empty' else (0, 1)
        for b in frames:
            assert torch.equal(out[b], d(under)[b]), what
        g = d(wgt).float()
        (out * g).sum().backward()
        for b in frames:
            assert torch.equal(u.grad[b], g[b]) and not a.grad[b].any() and all(not x.grad[b].any() for x in leaves), what
        if what == 'nf = 0':
            assert not p.grad.any()
        else:
            assert float(out[0].detach().sub(d(under)[0]).abs().max()) > 0 and not p.grad[1].any()


def check_entry_points_validate(dev):
    """argument errors come back as D3H_ERR_ARG, not as launches"""
    S = state(dev)
    t, L, R = _raw(dev, S, 0)
    lib = L.lib()
    p = lambda x: None if x is None else L._PTR(x.data_ptr())
    arr = lambda ts: (ctypes.c_void_p * len(ts))(*[None if x is None else x.data_ptr() for x in ts])
    ints = lambda v: (ctypes.c_int * len(v))(*v)
    out = torch.full_like(t['under'], float('nan'))
    ds = [torch.full((B, H, W, c), float('nan'), device=dev) for c in WIDTHS]

    def fwd(n=4, src='ok', nch=WIDTHS, kind=KINDS, under=t['under'], rast=t['rast'], pos=t['pos'], flags=t['flags'], o=out, nb=B, h=H):
        m = max(n, 1)
        srcs = None if src is None else arr((t['src'] * 4)[:m] if src == 'ok' else src)
        return lib.d3h_layer_composite_antialias_fwd(n, srcs, ints((list(nch) * 4)[:m]), ints((list(nch) * 4)[:m]),
                                                     ints((list(kind) * 4)[:m]), p(t['alpha']), p(under), p(rast), p(pos), R._bstride(t['pos']), p(t['tri']),
                                                     t['tri'].shape[0], p(flags), nb, h, W, p(o), L.stream())

    def bwd(n=4, kind=KINDS, under=t['under'], g=t['g'], dsrc='ok', dch=None):
        m = max(n, 1)
        return lib.d3h_layer_composite_antialias_bwd(n, arr((t['src'] * 4)[:m]), arr((ds * 4)[:m]) if dsrc == 'ok' else dsrc, dch, ints((list(WIDTHS) * 4)[:m]),
                                                     ints((list(WIDTHS) * 4)[:m]), ints((list(kind) * 4)[:m]), p(t['alpha']), p(under), p(t['rast']), p(t['pos']),
                                                     R._bstride(t['pos']), p(t['tri']), t['tri'].shape[0], p(t['flags']), B, H, W, p(g), None, None, None, L.stream())
    bad = [fwd(under=None), fwd(n=13), fwd(n=0), fwd(kind=(0, 4, 2, 3)), fwd(kind=(0, -1, 2, 3)), fwd(kind=(3, 1, 2, 3)), fwd(src=None),
           fwd(src=[t['src'][0], None, t['src'][2], t['src'][3]]), fwd(rast=None), fwd(o=None), fwd(o=t['under']), fwd(pos=None), fwd(flags=None),
           fwd(nb=-1), fwd(h=0), fwd(nch=(3, 0, 1, 1)),
           bwd(under=None), bwd(n=13), bwd(kind=(0, 1, 2, 7)), bwd(g=None), bwd(dch=ints((3, 2, 1, 1)))]
    assert bad == [-1] * len(bad), bad
    if dev != 'cpu':
        torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and all(bool(torch.isnan(x).all()) for x in ds), 'a refused call launched something'
    # more channels than a tile's rows have room for in LDS: refused, not launched
    wide = [t['src'][0]] * 12
    many = lib.d3h_layer_composite_antialias_fwd(12, arr(wide), ints([3] * 12), ints([7] * 12), ints([0] * 12), None, p(t['under']), p(t['rast']), p(t['pos']),
                                                 R._bstride(t['pos']), p(t['tri']), t['tri'].shape[0], p(t['flags']), B, H, W, p(out), L.stream())
    assert many == -1
    # the backward's limit counts the widest source gradient on its way out too: 62 channels pass forward and, without source gradients, backward;
    # with a source gradient of 5 they do not
    big, u62 = torch.zeros(B, H, W, 5, device=dev), torch.zeros(B, H, W, 62, device=dev)
    o62, d5 = torch.full_like(u62, float('nan')), torch.full_like(big, float('nan'))
    n62 = [4] * 10 + [5] * 2

    def wide_call(back, dsrc):
        common = (p(t['alpha']), p(u62), p(t['rast']), p(t['pos']), R._bstride(t['pos']), p(t['tri']), t['tri'].shape[0], p(t['flags']), B, H, W)
        if not back:
            return lib.d3h_layer_composite_antialias_fwd(12, arr([big] * 12), ints([5] * 12), ints(n62), ints([0] * 12), *common, p(o62), L.stream())
        return lib.d3h_layer_composite_antialias_bwd(12, arr([big] * 12), dsrc, None, ints([5] * 12), ints(n62), ints([0] * 12), *common, p(u62), None, None, None,
                                                     L.stream())
    assert wide_call(True, arr([None] * 11 + [d5])) == -1
    if dev != 'cpu':
        torch.cuda.synchronize()
    assert bool(torch.isnan(d5).all())
    assert wide_call(False, None) == 0 and wide_call(True, arr([None] * 12)) == 0
    if dev != 'cpu':
        torch.cuda.synchronize()
    assert bool(torch.isfinite(o62).all())                             # (launched: every entry written)
    assert fwd() == 0 and bwd() == 0 and bwd(dsrc=None) == 0 and fwd(nb=0) == 0
    if dev != 'cpu':
        torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()) and all(bool(torch.isfinite(x).all()) for x in ds)
    L._keepalive.clear()


# ---- 2. the layered render ---------------------------------------------------------------------------------------------------------------------
def check_render_buffers(dev, with_msdf):
    """every public buffer of render_mesh(num_layers=4) under FLAGS.transparency against the restatement, both routes, and the two against each other;
    with_msdf: all buffers plus msdf_image in one pass (the widest image)"""
    from render import render as rr
    S = state(dev)
    ex, mvp, cam, draws = S['ex'], S['mvp'], S['cam'], S['draws']
    extra = {'msdf': S['msdf'].to(dev)} if with_msdf else None
    every = sorted(rr.ALL_BUFFERS + rr.PERTURBED_BUFFERS + (('msdf_image',) if with_msdf else ()))
    keys = [k for k in rr.ALL_BUFFERS + ('msdf_image',) + rr.PERTURBED_BUFFERS if k in every]
    y64, y32 = yard(S, keys)
    with torch.no_grad():
        one = render(ex, mvp, cam, draws, layers=1, extra_dict=extra, _keep_rast=True)
        assert torch.equal(_cpu(one['_rast']), S['rasts'][0])
        outs = {}
        for fused in (True, False):
            (out, n) = routes_taken(lambda: render(ex, mvp, cam, draws, fused=fused, extra_dict=extra, _keep_rast=True))
            steps = LAYERS * (2 if len(keys) > 12 else 1)
            assert n == ({'fused': steps, 'composed': 0} if fused else {'fused': 0, 'composed': steps}), n
            assert _public(out) == every
            assert torch.equal(out['visible_triangles'], one['visible_triangles']) and torch.equal(out['_rast'], one['_rast'])
            what = 'fused' if fused else 'composed'
            for k in keys:
                assert out[k].shape == y64[k].shape, (k, out[k].shape)
                assert_close(f'{k} [{what}] vs float64', out[k], y64[k], y32[k])
            outs[fused] = out
        for k in keys:
            tol = max(5.0 * rel(y32[k], y64[k]), FLOOR)
            r = rel(outs[True][k], outs[False][k])
            print(f'{k} fused vs composed: {r:.3e} (bound {tol:.3e})')
            assert r <= tol, (k, r, tol)
        # the layers are there: the blended opacity exceeds the first layer's, and differs from the one-layer render
        a4, a1 = outs[True]['kd'][..., 3], one['kd'][..., 3]
        assert float(a4.max()) > float(a1.max()) + 0.05 and float(a4.max()) <= 1.0


# ---- 3. gradients ------------------------------------------------------------------------------------------------------------------------------
def _loss_weights():
    g = torch.Generator().manual_seed(43)
    return torch.rand(2, B, H, W, 3, generator=g, dtype=torch.float64) + 0.5      # every pixel, silhouettes included


def check_map_gradients(dev, fused):
    """d(sum(w shaded) + sum(w' normal) + sum(w' ks)) / d(kd map with its alpha channel, ks map, normal map) against float64 autograd of the restatement
    (ks reaches neither shaded nor normal: a ks term is added so that its gradient is checked at all, as tests/texmat_cases.py does)"""
    S = state(dev)
    ex, mvp, cam, draws = S['ex'], S['mvp'], S['cam'], S['draws']
    names = ('kd', 'ks', 'normal')
    for k in names:
        ex.material[k].data.grad = None
    keys = ('shaded', 'normal', 'ks')
    (out, n) = routes_taken(lambda: render(ex, mvp, cam, draws, fused=fused, buffers=keys))
    assert n == ({'fused': LAYERS, 'composed': 0} if fused else {'fused': 0, 'composed': LAYERS}), n
    w = _loss_weights()
    wd = w.float().to(dev)
    ((out['shaded'][..., :3] * wd[0]).sum() + (out['normal'][..., :3] * wd[1]).sum() + (out['ks'][..., :3] * wd[1]).sum()).backward()
    ref = {}
    for dt in (torch.float64, torch.float32):
        ms = [_cpu(ex.material[k].data).to(dt).clone().requires_grad_(True) for k in names]
        y = y_render(S, dt, keys, maps=ms)
        ((y['shaded'][..., :3] * w[0].to(dt)).sum() + (y['normal'][..., :3] * w[1].to(dt)).sum() + (y['ks'][..., :3] * w[1].to(dt)).sum()).backward()
        ref[dt] = [m.grad for m in ms]
    what = 'fused' if fused else 'composed'
    for i, k in enumerate(names):
        got = ex.material[k].data.grad
        assert got is not None and float(got.abs().sum()) > 0, f'no gradient reaches the {k} map'
        assert_close(f'd loss / d {k} map [{what}] vs float64 autograd', got, ref[torch.float64][i], ref[torch.float32][i])
    ga = ex.material['kd'].data.grad[..., 3]
    assert float(ga.abs().max()) > 0
    assert_close(f'd loss / d alpha channel [{what}]', ga, ref[torch.float64][0][..., 3], ref[torch.float32][0][..., 3])
    for k in names:
        ex.material[k].data.grad = None


def check_position_gradient(dev, fused):
    """d loss / d v_pos (the lookups take the composed route, as in tests/texmat_cases.py:check_position_gradient) against float64 autograd of the
    restatement in which barycentrics, texel coordinates, opacity and the silhouette crossings are functions of the positions"""
    from render import mesh as rmesh
    S = state(dev)
    ex, mvp, cam, draws = S['ex'], S['mvp'], S['cam'], S['draws']
    pos = ex.v_pos.detach().clone().requires_grad_(True)
    m = rmesh.Mesh(pos, base=ex)
    keys = ('shaded', 'normal')
    (out, n) = TC.routes_taken(lambda: render(m, mvp, cam, draws, fused=fused, buffers=keys))
    assert n == {'fused': 0, 'composed': LAYERS}, n
    w = _loss_weights()
    wd = w.float().to(dev)
    ((out['shaded'][..., :3] * wd[0]).sum() + (out['normal'][..., :3] * wd[1]).sum()).backward()
    ref = {}
    for dt in (torch.float64, torch.float32):
        p = _cpu(ex.v_pos).to(dt).clone().requires_grad_(True)
        y = y_render(S, dt, keys, v_pos=p)
        ((y['shaded'][..., :3] * w[0].to(dt)).sum() + (y['normal'][..., :3] * w[1].to(dt)).sum()).backward()
        ref[dt] = p.grad
    assert float(ref[torch.float64].abs().max()) > 0
    assert_close(f"d loss / d v_pos [{'fused' if fused else 'composed'} blend] vs float64 autograd", pos.grad, ref[torch.float64], ref[torch.float32])
    for k in ('kd', 'ks', 'normal'):
        ex.material[k].data.grad = None


# ---- 4. exactness ------------------------------------------------------------------------------------------------------------------------------
def check_exactness(dev):
    from render import render as rr
    S = state(dev)
    ex, mvp, cam, draws = S['ex'], S['mvp'], S['cam'], S['draws']
    with torch.no_grad():
        for fused in (True, False):
            four = render(ex, mvp, cam, draws, fused=fused)
            six = render(ex, mvp, cam, draws, layers=6, fused=fused)
            assert _public(six) == _public(four)
            for k in _public(four):
                assert torch.equal(six[k], four[k]), (k, fused)
            assert torch.equal(six['visible_triangles'], four['visible_triangles'])
        # opacity 0 everywhere over a constant background: every buffer is its background
        clear, _, _, _ = scene(dev, alpha=0.0)
        bg = torch.full((1, H, W, 3), 0.3, device=dev)
        for fused in (True, False):
            out = render(clear, mvp, cam, draws, fused=fused, background=bg)
            for k in _public(out):
                t = out[k]
                if k == 'shaded':
                    want = torch.cat((bg.expand(B, H, W, 3), torch.zeros(B, H, W, 1, device=dev)), dim=-1)
                elif k == 'depth':
                    want = torch.full_like(t, 20.0)
                else:
                    want = torch.zeros_like(t)
                assert torch.equal(t, want), (k, fused)
        # FLAGS.transparency with a 3-channel kd and one layer: the render without the flag
        _, ex3, mvp3, cam3, draws3 = TC.scene(dev)
        off = render(ex3, mvp3, cam3, draws3, layers=1, transparency=False)
        (on, n) = routes_taken(lambda: render(ex3, mvp3, cam3, draws3, layers=1, transparency=True))
        assert n == {'fused': 0, 'composed': 0} and _public(on) == _public(off)
        for k in _public(off):
            assert torch.equal(on[k], off[k]), k
        # one layer without the flag: the single-layer code, whatever the layer switches say -- no blend step of either route runs, the same bits
        for flags in (_Flags(), _Flags(transparency=False)):
            for fused in (None, True, False):
                (again, n) = routes_taken(lambda: render(ex3, mvp3, cam3, draws3, layers=1, flags=flags, fused=fused))
                assert n == {'fused': 0, 'composed': 0}
                for k in _public(off):
                    assert torch.equal(again[k], off[k]), k
                assert torch.equal(again['visible_triangles'], off['visible_triangles'])
        (mlp, n) = routes_taken(lambda: TC.render(TC.scene(dev)[0], TC.scene(dev)[0], mvp3, cam3, draws3, use_uv=False))
        assert n == {'fused': 0, 'composed': 0} and _public(mlp) == sorted(rr.ALL_BUFFERS)


# ---- 5. options and errors ---------------------------------------------------------------------------------------------------------------------
def check_options_and_errors(dev):
    from render import mesh as rmesh, texture as RT
    S = state(dev)
    ex, mvp, cam, draws = S['ex'], S['mvp'], S['cam'], S['draws']
    with torch.no_grad():
        full = render(ex, mvp, cam, draws)
        only = render(ex, mvp, cam, draws, buffers=('shaded',))
        assert _public(only) == ['shaded'] and torch.equal(only['shaded'], full['shaded'])
    live = render(ex, mvp, cam, draws, _grad_buffers=('shaded',))
    assert live['shaded'].requires_grad and not live['kd_grad'].requires_grad and not live['normal'].requires_grad
    assert set(live['_layout']) == {'shaded'} and live['_stacked'].shape[-1] == 4 and not live['_stacked_nograd'].requires_grad
    assert torch.equal(live['shaded'].detach(), full['shaded']) and torch.equal(live['normal'], full['normal'])
    with torch.no_grad():
        for msaa in (True, False):
            o = render(ex, mvp, cam, None, spp=2, msaa=msaa)
            for k in _public(o):
                assert o[k].shape[:3] == (B, H, W) and bool(torch.isfinite(o[k]).all()), (k, msaa)
            assert o['kd'].shape == (B, H, W, 4) and float(o['kd'][..., 3].max()) <= 1.0 and float(o['kd'][..., 3].max()) > 0.9
        # opaque layers need no flag: a 3-channel kd, two layers
        _, ex3, mvp3, cam3, draws3 = TC.scene(dev)
        (o3, n) = routes_taken(lambda: render(ex3, mvp3, cam3, draws3, layers=2, transparency=False, buffers=('kd',)))
        assert n['fused'] + n['composed'] == 2
        o1 = render(ex3, mvp3, cam3, draws3, layers=1, transparency=False, buffers=('kd', '_rast'))
        ins = TC.interior(o1['_rast'])              # (a silhouette pixel blends with what lies behind it: the back layer now, the background before)
        assert int(ins.sum()) > 200 and torch.equal(o3['kd'].cpu()[ins], o1['kd'].cpu()[ins]), 'an opaque front layer does not hide the back layer'
        assert float((o3['kd'] - o1['kd']).abs().max()) > 0.01
    # the opacity weighs every buffer: it gets its gradient through a buffer that reads no map at all
    ex.material['kd'].data.grad = None
    dep = render(ex, mvp, cam, draws, buffers=('depth',), _grad_buffers=('depth',))
    wd = _loss_weights()[0, ..., :2]
    (dep['depth'] * wd.float().to(dev)).sum().backward()
    got = ex.material['kd'].data.grad
    assert got is not None and float(got[..., 3].abs().max()) > 0 and not got[..., :3].any()
    ref = []
    for dt in (torch.float64, torch.float32):
        ms = [_cpu(ex.material[k].data).to(dt).clone().requires_grad_(k == 'kd') for k in ('kd', 'ks', 'normal')]
        (y_render(S, dt, ('depth',), maps=ms)['depth'] * wd.to(dt)).sum().backward()
        ref.append(ms[0].grad[..., 3])
    assert_close("d sum(w depth) / d alpha channel, _grad_buffers=('depth',)", got[..., 3], ref[0], ref[1])
    ex.material['kd'].data.grad = None
    with pytest.raises(ValueError, match='num_layers'):
        render(ex, mvp, cam, draws, layers=0)
    with pytest.raises(NotImplementedError, match='lit_shading'):
        render(ex, mvp, cam, draws, flags=_Flags(transparency=True, lit_shading=True), bsdf='pbr')
    with pytest.raises(NotImplementedError, match='transparency'):
        render(ex, mvp, cam, draws, transparency=False)
    with pytest.raises(NotImplementedError, match='transparency'):
        four = rmesh.Mesh(base=ex3)
        four.material = dict(ex3.material, kd=RT.Texture2D(torch.ones(1, 4, 4, 4, device=dev)))
        render(four, mvp3, cam3, draws3, layers=1, transparency=False)


def check_export_options(dev):
    """d3h.export.textured_mesh(transparency=..., alpha_init=...)"""
    from d3h import export
    base = TC.scene(dev)[0]
    args = (base, base.material, 32, [-1.0] * 3, [1.0] * 3, [-1.0] * 3, [1.0] * 3, [-1.0, -1.0, 0.0], [1.0, 1.0, 1.0])
    plain = export.textured_mesh(*args)
    assert plain.material['kd'].data.shape[-1] == 3 and len(plain.material['kd'].min_max[0]) == 3
    half = export.textured_mesh(*args, transparency=True, alpha_init=0.5)
    assert torch.equal(half.material['kd'].data[..., :3], plain.material['kd'].data) and bool((half.material['kd'].data[..., 3] == 0.5).all())
    assert export.textured_mesh(*args, transparency=False, alpha_init=0.5).material['kd'].data.shape[-1] == 3
    rnd = export.textured_mesh(*args, transparency=True, alpha_init='rand').material['kd'].data[..., 3].detach()
    assert 0.0 <= float(rnd.min()) < 0.1 and 0.9 < float(rnd.max()) < 1.0 and abs(float(rnd.mean()) - 0.5) < 0.05
    own = export.textured_mesh(base, base.material, 32, [0.0, 0.0, 0.0, 0.25], [1.0, 1.0, 1.0, 0.75], *args[5:], transparency=True)
    assert [float(x) for x in own.material['kd'].min_max[0]] == [0.0, 0.0, 0.0, 0.25] and float(own.material['kd'].min_max[1][3]) == 0.75
    with pytest.raises(ValueError, match='alpha_init'):
        export.textured_mesh(*args, transparency=True, alpha_init='noise')


# ---- 6. round trip -----------------------------------------------------------------------------------------------------------------------------
def check_round_trip(dev, tmp_path):
    """write_obj writes an RGBA texture_kd.png (colour sRGB, opacity linear), load_textured_mesh reads four channels back, and the layered render of
    the file is within the PNG's quantisation of the original's.  The bound: a stored colour moves by at most `step` (half an 8-bit sRGB step at 1, the
    steepest: tests/texmat_cases.py:check_round_trip), a stored opacity by half a linear step, both plus the uv text round trip TEX 2^-23.  A buffer
    is sum_l T_l a_l c_l with T_l = prod_{m<l} (1 - a_m) and sum_l T_l a_l <= 1: the colours contribute at most `step`.  d out / d a_l = T_l (c_l -
    what lies behind); what lies behind is a blend of colours and the zero background, so |c_l - behind| <= cmax, the largest stored colour, and with
    every opacity >= amin (0.2 here) T_l <= (1 - amin)^l: the four opacities contribute at most cmax sum_l (1 - amin)^l half steps (2.5, not 4).  The
    buffers' own opacity channel, 1 - prod (1 - a_l), moves by at most 4 (1 - amin)^3 = 2.05 half steps, which is less.  Antialias blends cannot widen
    it.  The opacity map read back is also compared directly: an opacity decoded as sRGB would be off by up to 0.1."""
    from d3h import export
    from render import obj, util
    ex, mvp, cam, draws = scene(dev)
    with torch.no_grad():
        ex.material['kd'].data[..., :3] = ex.material['kd'].data[..., :3] * 0.6 + 0.5           # colours a PNG can hold
        ex.material['ks'].data.copy_(ex.material['ks'].data * 0.6 + 0.5)
        obj.write_obj(str(tmp_path), ex)
        png = util.load_image(os.path.join(str(tmp_path), 'texture_kd.png'))
        assert png.shape == (TEX, TEX, 4)
        a_err = float((torch.from_numpy(png[..., 3]) - _cpu(ex.material['kd'].data)[0, ..., 3]).abs().max())
        assert a_err <= 0.5 / 255 + 1e-7, 'the opacity is not stored linearly'
        back = export.load_textured_mesh(os.path.join(str(tmp_path), 'mesh.obj'), device=dev)
        assert tuple(back.material['kd'].data.shape) == (1, TEX, TEX, 4) and back.material['filter_mode'] == 'linear'
        a_back = float((back.material['kd'].data[..., 3] - ex.material['kd'].data[..., 3]).abs().max())
        print(f'opacity map read back: off by {a_back:.3e} (bound {0.5 / 255 + 1e-7:.3e})')
        assert a_back <= 0.5 / 255 + 1e-7, 'the opacity does not come back linearly'
        a = render(ex, mvp, cam, draws, buffers=('kd', 'shaded'))
        b = render(back, mvp, cam, draws, buffers=('kd', 'shaded'))
        one = torch.ones(1, dtype=torch.float64)
        step = float(util.srgb_to_rgb(one) - util.srgb_to_rgb(one - 0.5 / 255))
        uv = TEX * 2.0 ** -23
        amin, cmax = float(ex.material['kd'].data[..., 3].min()), float(ex.material['kd'].data[..., :3].max())
        assert amin >= 0.2 and 0.5 < cmax <= 1.0
        bound = (step + uv) + cmax * sum((1.0 - amin) ** l for l in range(LAYERS)) * (0.5 / 255 + uv) + 1e-6
        for k in ('kd', 'shaded'):
            d = float((a[k] - b[k]).abs().max())
            print(f'round trip {k}: off by {d:.3e} (bound {bound:.3e})')
            assert 0 < d <= bound
