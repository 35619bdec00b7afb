"""Check functions of the lit render path -- the light's sampling tables (csrc/envlight.hip, d3h/envlight.py, render/light.py), the denoiser module
and its two-image kernel (csrc/denoise.hip, d3h/denoise.py, denoiser/denoiser.py), render.render.shade_lit, the FLAGS.lit_shading branch of
render_mesh and one lit tick_init -- shared by tests/test_lit_emul.py (host emulation of the kernel sources) and tests/test_gpu_lit.py (MI355X).
Same shapes on both; every fixture is generated here from a seed or taken from tests/optixutils_cases.py.

Parity rule of the tables: the project's (optixutils_cases.assert_close): max|got - f64| / max|f64| <= max(5 x the error of the float32 twin,
2^-20), f64 the formulas of render/light.py:46-59 in float64, the twin optixutils_cases.light_tables.  Everything else here is an identity between
two ways of running the same kernels and is held bit for bit, except the light's gradient, which float atomics sum in an order that varies: 1e-5
of its maximum, the bound parity_cases.py uses for d(pos) of the antialias pass."""
import functools
import json
import os
import types

import numpy as np
import pytest
import torch

import optixutils_cases as OC
from conftest import GOLD

_to = OC._to

# ---- light tables --------------------------------------------------------------------------------------------------------------------------
LIGHT_MAPS = ('1x1', '5x7', '16x16', '33x130', '64x300')
TALL_MAPS = ('300x5',)             # more rows than threads of a workgroup: the row table's segments are two rows long
ZERO_ROW = 17                      # of the 64 x 300 map


@functools.lru_cache(maxsize=None)
def light_map(name):
    H, W = (int(v) for v in name.split('x'))
    rng = np.random.default_rng(1000 * H + W)
    base = rng.uniform(0.05, 4.0, (H, W, 3)).astype(np.float32)
    if name == '16x16':            # a single bright texel: 15 rows without any light
        base[:] = 0.0
        base[5, 9] = (3.0, 1.0, 2.0)
    if name == '64x300':
        base[ZERO_ROW] = 0.0
    return base


@functools.lru_cache(maxsize=None)
def light_reference(name):
    """(pdf, rows [H], cols) in float64 by the formulas of render/light.py:46-59, and the float32 twin"""
    base = light_map(name)
    b = base.astype(np.float64)
    H, W = b.shape[:2]
    pdf = b.max(-1) * np.sin((np.arange(H, dtype=np.float64) + 0.5) / H * np.pi)[:, None]
    pdf = pdf / pdf.sum()
    cols = np.cumsum(pdf, 1)
    rows = np.cumsum(cols[:, -1])
    cols = cols / np.where(cols[:, -1:] > 0, cols[:, -1:], 1.0)
    rows = rows / (rows[-1] if rows[-1] > 0 else 1.0)
    p32, r32, c32 = OC.light_tables(base)
    return (pdf, rows, cols), (p32, r32[:, 0], c32)


def check_light_tables(dev, name):
    from d3h import envlight as EL
    from render import light
    base = light_map(name)
    H, W = base.shape[:2]
    (p64, r64, c64), (p32, r32, c32) = light_reference(name)
    t = _to(dev, base)
    pdf, rows, cols = EL.tables(t)
    again = EL.tables(t)
    assert tuple(pdf.shape) == tuple(rows.shape) == tuple(cols.shape) == (H, W) and pdf.dtype == rows.dtype == cols.dtype == torch.float32
    assert not pdf.requires_grad and torch.equal(rows, rows[:, :1].expand(H, W))
    for a, b in zip((pdf, rows, cols), again):
        assert torch.equal(a, b), 'two runs differ'
    OC.assert_close(f'light {name}: pdf', pdf, p64, p32)
    OC.assert_close(f'light {name}: rows', rows[:, 0], r64, r32)
    OC.assert_close(f'light {name}: cols', cols, c64, c32)
    # what the sampler's search relies on, exactly
    r, c, p = rows[:, 0].cpu(), cols.cpu(), pdf.cpu()
    assert (p >= 0).all()
    assert (r[1:] >= r[:-1]).all() and (c[:, 1:] >= c[:, :-1]).all(), 'a table decreases'
    assert float(r[-1]) == 1.0
    lit_rows = torch.from_numpy(c64[:, -1] > 0)
    assert (c[lit_rows, -1] == 1.0).all() and (c[~lit_rows] == 0).all()
    if name == '64x300':
        assert not bool(lit_rows[ZERO_ROW]) and (c[ZERO_ROW] == 0).all() and float(r[ZERO_ROW]) == float(r[ZERO_ROW - 1])
    if name == '16x16':
        assert int(lit_rows.sum()) == 1 and float(p[5, 9]) == 1.0 and float(p.sum()) == 1.0
    # the module runs the same kernel on the live parameter
    lgt = light.EnvironmentLight(t.clone().requires_grad_(True))
    assert torch.equal(lgt._pdf, pdf) and torch.equal(lgt.rows, rows) and torch.equal(lgt.cols, cols)
    assert torch.equal(lgt.rows[:, 0], rows[:, 0]) and not lgt._pdf.requires_grad
    with torch.no_grad():
        lgt.base.mul_(0.5).add_(0.125)
    lgt.update_pdf()
    for a, b in zip((lgt._pdf, lgt.rows, lgt.cols), EL.tables(lgt.base)):
        assert torch.equal(a, b)
    assert not torch.equal(lgt._pdf, pdf) or name == '1x1'


def check_light_validation(dev):
    from d3h import envlight as EL
    for shape in ((4, 4), (4, 4, 4), (0, 4, 3)):
        with pytest.raises(RuntimeError):
            EL.tables(torch.zeros(*shape, device=dev))


# ---- light module ----------------------------------------------------------------------------------------------------------------------------
def check_light_module(dev):
    from render import light
    surface = json.load(open(os.path.join(GOLD, 'light_surface.json')))
    public = sorted(k for k, v in vars(light).items() if not k.startswith('_') and getattr(v, '__module__', None) == light.__name__)
    assert public == sorted(surface['module']), public
    cls = light.EnvironmentLight
    assert sorted(k for k in vars(cls) if not k.startswith('__')) == sorted(surface['class']), sorted(vars(cls))
    lgt = light.create_trainable_env_rnd(16)
    assert sorted(vars(lgt)) == sorted(surface['instance']), sorted(vars(lgt))
    assert (cls.LIGHT_MIN_RES, cls.MIN_ROUGHNESS, cls.MAX_ROUGHNESS) == (16, 0.08, 0.5)
    assert tuple(lgt.base.shape) == (16, 16, 3) and lgt.base.requires_grad and lgt.base.is_leaf and lgt.parameters()[0] is lgt.base
    assert float(lgt.base.detach().min()) >= 0.25 and float(lgt.base.detach().max()) <= 0.75 and lgt.mtx is None
    assert abs(lgt.pdf_scale - 256 / (2 * np.pi * np.pi)) < 1e-9
    lgt.xfm('m')
    assert lgt.mtx == 'm'
    c = lgt.clone()
    assert isinstance(c, cls) and not c.base.requires_grad and c.base.data_ptr() != lgt.base.data_ptr() and torch.equal(c.base, lgt.base.detach())
    assert torch.equal(c._pdf, lgt._pdf)
    with torch.no_grad():
        lgt.base[0, 0, 0], lgt.base[1, 1, 1] = -1.0, 9.0
        before = lgt.base.data_ptr()
        lgt.clamp_(min=1e-4, max=5.0)
    assert lgt.base.data_ptr() == before and float(lgt.base.detach()[0, 0, 0]) == np.float32(1e-4) and float(lgt.base.detach()[1, 1, 1]) == 5.0
    img = lgt.generate_image([6, 10])
    assert tuple(img.shape) == (6, 10, 3) and not img.requires_grad and torch.isfinite(img).all()
    same = lgt.generate_image([16, 16])                        # texel centres: the bilinear lookup returns the map
    assert (same - lgt.base.detach()).abs().max() <= 1e-6 * 5.0


def check_light_files(dev, tmp_path):
    """load_env (through util.load_image) and save_env_map"""
    from render import light, util
    from d3h.checkpoint import write_hdr
    rng = np.random.default_rng(5)
    mant = rng.integers(0, 256, (6, 9, 3))
    mant[..., 1] = rng.integers(128, 256, (6, 9))
    env = (mant * 2.0 ** (rng.integers(-3, 3, (6, 9, 1)) - 8)).astype(np.float32)          # 8-bit mantissas under the pixel's exponent: what RGBE holds exactly
    env[2, 3] = 0.0
    fn = str(tmp_path / 'probe.hdr')
    write_hdr(fn, env)
    assert np.array_equal(util.load_image(fn), env)
    lgt = light.load_env(fn, scale=2.0)
    assert isinstance(lgt, light.EnvironmentLight) and lgt.base.device.type == torch.device(dev).type and not lgt.base.requires_grad
    assert torch.equal(lgt.base.cpu(), torch.from_numpy(env * 2.0)) and tuple(lgt._pdf.shape) == (6, 9) and float(lgt.rows[-1, 0]) == 1.0
    small = light.load_env(fn, res=[4, 5], trainable=True)
    assert tuple(small.base.shape) == (4, 5, 3) and small.base.requires_grad and small.base.is_leaf
    b = small.base.detach()
    assert float(b.min()) >= np.float32(0.0001) and float(b.max()) <= float(env.max()) and abs(small.pdf_scale - 20 / (2 * np.pi * np.pi)) < 1e-9
    with pytest.raises(AssertionError):
        light.load_env(str(tmp_path / 'probe.exr'))
    out = str(tmp_path / 'saved.hdr')
    light.save_env_map(out, lgt)
    saved = util.load_image(out if os.path.exists(out) else out + '.npy')          # the raw array where no image library writes .hdr
    want = lgt.generate_image([512, 1024]).cpu().numpy()
    assert saved.shape == (512, 1024, 3) and np.abs(saved - want).max() <= 2.0 ** -8 * want.max()          # 8 bits of mantissa at the most
    with pytest.raises(AssertionError):
        light.save_env_map(out, env)


# ---- denoiser pair ---------------------------------------------------------------------------------------------------------------------------
def _denoise_inputs(dev, shape):
    fx = OC.denoise_fixture(shape)
    rng = np.random.default_rng(31 + shape[2])
    b = rng.uniform(0.0, 3.0, fx['col'].shape).astype(np.float32)
    gb = rng.standard_normal(fx['g'].shape).astype(np.float32)
    return fx, b, gb


def check_denoiser_pair(dev, shape, sigma):
    from d3h import denoise as DN
    fx, b_np, gb_np = _denoise_inputs(dev, shape)
    nrm, zdz = _to(dev, fx['nrm']), _to(dev, fx['zdz'])
    single = []
    for col, g in ((fx['col'], fx['g']), (b_np, gb_np)):
        c = _to(dev, col, True)
        o = DN.bilateral_denoise(c, nrm, zdz, sigma)
        o.backward(_to(dev, g))
        single.append((o.detach(), c.grad))
    a, b = _to(dev, fx['col'], True), _to(dev, b_np, True)
    nrm_g, zdz_g = _to(dev, fx['nrm'], True), _to(dev, fx['zdz'], True)
    oa, ob = DN.bilateral_denoise_many([a, b], nrm_g, zdz_g, sigma)
    torch.autograd.backward([oa, ob], [_to(dev, fx['g']), _to(dev, gb_np)])
    assert nrm_g.grad is None and zdz_g.grad is None
    assert float(single[0][0].abs().max()) > 0 and not torch.equal(single[0][0], single[1][0])
    for what, got, ref in (('out a', oa.detach(), single[0][0]), ('out b', ob.detach(), single[1][0]), ('d a', a.grad, single[0][1]), ('d b', b.grad, single[1][1])):
        assert got.shape == ref.shape and torch.equal(got, ref), (what, float((got - ref).abs().max()))
    # only one of the two is differentiated
    a2 = _to(dev, fx['col'], True)
    oa2, ob2 = DN.bilateral_denoise_many([a2, _to(dev, b_np)], nrm, zdz, sigma)
    oa2.backward(_to(dev, fx['g']))
    assert torch.equal(a2.grad, single[0][1]) and torch.equal(ob2, single[1][0])
    # a list of one
    a1 = _to(dev, fx['col'], True)
    (o1,) = DN.bilateral_denoise_many([a1], nrm, zdz, sigma)
    o1.backward(_to(dev, fx['g']))
    assert torch.equal(o1.detach(), single[0][0]) and torch.equal(a1.grad, single[0][1])


def check_denoiser_module(dev, shape):
    from denoiser.denoiser import BilateralDenoiser
    from render import util
    import render.optixutils as ou
    fx, b_np, _ = _denoise_inputs(dev, shape)
    d = BilateralDenoiser(influence=0.5)
    assert isinstance(d, torch.nn.Module) and (d.sigma, d.variance, d.N) == (1.0, 1.0, 7)
    d.set_influence(0.0)
    assert (d.sigma, d.N) == (0.0001, 3) and d.variance == 0.0001 ** 2.
    d.set_influence(1.0)
    assert (d.sigma, d.variance, d.N) == (2.0, 4.0, 11)
    d.set_influence(0.5)
    bent = fx['nrm'] * np.linspace(0.4, 1.0, fx['nrm'].shape[2], dtype=np.float32)[None, None, :, None]          # shorter than 1, as bent normals are
    col, nrm, zdz = _to(dev, fx['col']), _to(dev, bent), _to(dev, fx['zdz'])
    out = d(torch.cat((col, nrm, zdz), dim=-1))
    ref = ou.bilateral_denoiser(col, util.safe_normalize(nrm), zdz, 1.0)
    assert tuple(out.shape) == (*shape, 3) and torch.equal(out, ref)
    assert not torch.equal(out, ou.bilateral_denoiser(col, nrm, zdz, 1.0)), 'the normals were not normalised'
    many = d.forward_many([col, _to(dev, b_np)], nrm, zdz)
    assert len(many) == 2 and torch.equal(many[0], out) and torch.equal(many[1], d(torch.cat((_to(dev, b_np), nrm, zdz), dim=-1)))
    (one,) = d.forward_many([col], nrm, zdz)
    assert torch.equal(one, out)


def check_denoiser_pair_validation(dev):
    from d3h import denoise as DN
    z = lambda *s: torch.zeros(*s, device=dev)
    ok = (z(1, 4, 4, 3), z(1, 4, 4, 3), z(1, 4, 4, 2))
    for cols, nrm, zdz, sigma in (([ok[0]] * 3, ok[1], ok[2], 1.0), ([], ok[1], ok[2], 1.0), ([ok[0], z(1, 4, 5, 3)], ok[1], ok[2], 1.0),
                                  ([ok[0], ok[0]], ok[1], z(1, 4, 4, 3), 1.0), ([ok[0], ok[0]], z(1, 4, 4, 2), ok[2], 1.0),
                                  ([ok[0], ok[0]], ok[1], ok[2], 0.0), ([ok[0]], ok[1], ok[2], -1.0)):
        with pytest.raises(RuntimeError):
            DN.bilateral_denoise_many(cols, nrm, zdz, sigma)


# ---- shade_lit -------------------------------------------------------------------------------------------------------------------------------
N_SHADE = 2
SEED0 = 4321


def _flags(**kw):
    f = dict(n_samples=N_SHADE, decorrelated=False, denoiser_demodulate=True)
    f.update(kw)
    return types.SimpleNamespace(**f)


def _shade_inputs(dev):
    """leaves of one run: OC.shade_fixture's g-buffer, a light with tables, a context over the fixture's scene, (z, |dz|) and three cotangents"""
    from render import light
    import render.optixutils as ou
    fx = OC.shade_fixture(N_SHADE)
    rng = np.random.default_rng(99)
    shp = fx['pos'].shape[:3]
    zdz = np.stack([2.0 + rng.uniform(-0.2, 0.2, shp), rng.uniform(0.01, 1.0, shp)], -1).astype(np.float32)
    g = [rng.standard_normal(fx['pos'].shape).astype(np.float32) for _ in range(3)]
    ins = dict(pos=_to(dev, fx['pos'], True), nrm=_to(dev, fx['nrm'], True), kd=_to(dev, fx['kd'], True), ks=_to(dev, fx['ks'], True))
    lgt = light.EnvironmentLight(_to(dev, fx['light'], True))
    ctx = ou.OptiXContext()
    ou.optix_build_bvh(ctx, _to(dev, fx['verts']), _to(dev, fx['tris']), rebuild=1)
    const = dict(mask=_to(dev, fx['mask']), ro=_to(dev, fx['ro']), view=_to(dev, fx['view'][:, :1, :1]), zdz=_to(dev, zdz), g=[_to(dev, t) for t in g])
    return ins, lgt, ctx, const


def _grads(ins, lgt, outs, g):
    torch.autograd.backward([outs['shaded'], outs['diffuse_light'], outs['specular_light']], g)
    return {**{k: v.grad for k, v in ins.items()}, 'light': lgt.base.grad}


def check_shade_lit(dev, bsdf, demodulate):
    from render import render as R, util
    from denoiser.denoiser import BilateralDenoiser
    import render.optixutils as ou
    den = BilateralDenoiser(influence=0.5)
    F = _flags(denoiser_demodulate=demodulate)
    # the function under test
    ins, lgt, ctx, c = _shade_inputs(dev)
    R.rnd_seed = SEED0
    got = R.shade_lit(F, c['mask'], c['ro'], ins['pos'], ins['nrm'], c['zdz'], c['view'], ins['kd'], ins['ks'], lgt, ctx, bsdf, den, 0.75)
    assert R.rnd_seed == SEED0 + 1 and sorted(got) == ['diffuse_light', 'shaded', 'specular_light']
    d_got = _grads(ins, lgt, got, c['g'])
    # op by op
    ins, lgt, ctx, c = _shade_inputs(dev)
    kd = torch.ones_like(ins['kd']) if bsdf == 'white' else ins['kd']
    diff, spec = ou.optix_env_shade(ctx, c['mask'], c['ro'], ins['pos'], ins['nrm'], c['view'].expand(ins['pos'].shape), kd, ins['ks'], lgt.base, lgt._pdf,
                                    lgt.rows[:, 0], lgt.cols, BSDF=bsdf, n_samples_x=N_SHADE, rnd_seed=SEED0, shadow_scale=0.75)
    n1 = util.safe_normalize(ins['nrm'])
    if demodulate:
        diff, spec = ou.bilateral_denoiser(diff, n1, c['zdz'], den.sigma), ou.bilateral_denoiser(spec, n1, c['zdz'], den.sigma)
    shaded = kd * (1.0 - ins['ks'][..., 2:3]) * diff + spec if bsdf == 'pbr' else diff * kd
    if not demodulate:
        shaded = ou.bilateral_denoiser(shaded, n1, c['zdz'], den.sigma)
    ref = {'shaded': shaded, 'diffuse_light': diff, 'specular_light': spec}
    d_ref = _grads(ins, lgt, ref, c['g'])
    for k in ref:
        assert tuple(got[k].shape) == tuple(ref[k].shape) == (2, 9, 13, 3)
        assert torch.equal(got[k], ref[k]), (bsdf, demodulate, k, float((got[k] - ref[k]).abs().max()))
    assert float(got['diffuse_light'].detach().abs().max()) > 0 and (bsdf != 'pbr' or float(got['specular_light'].detach().abs().max()) > 0)
    for k in ('pos', 'nrm', 'kd', 'ks'):
        assert (d_got[k] is None) == (d_ref[k] is None), k
        if d_ref[k] is not None:
            assert torch.equal(d_got[k], d_ref[k]), (bsdf, demodulate, k, float((d_got[k] - d_ref[k]).abs().max()))
    assert d_ref['nrm'] is not None and float(d_ref['nrm'].abs().max()) > 0 and (bsdf == 'white') == (d_ref['kd'] is None)
    err, top = float((d_got['light'] - d_ref['light']).abs().max()), float(d_ref['light'].abs().max())
    print(f'shade_lit {bsdf} demodulate={demodulate}: d(light) differs by {err:.3e} of max {top:.3e} (bound 1e-5 of it)')
    assert top > 0 and err <= 1e-5 * top


def check_shade_lit_seed_and_denoiser_paths(dev, monkeypatch):
    """the seed counter, FLAGS.decorrelated, a denoiser without forward_many, no denoiser, one context per frame, argument errors"""
    from render import render as R
    from denoiser.denoiser import BilateralDenoiser
    import render.optixutils as ou
    ins, lgt, ctx, c = _shade_inputs(dev)
    seen = []
    real = ou.optix_env_shade

    def spy(*a, **kw):
        seen.append((a[0], kw['rnd_seed'], tuple(a[1].shape)))
        return real(*a, **kw)
    monkeypatch.setattr(R.ou, 'optix_env_shade', spy)
    den = BilateralDenoiser(influence=0.5)
    run = lambda F, ctx_=ctx, den_=den, bsdf='pbr': R.shade_lit(F, c['mask'], c['ro'], ins['pos'], ins['nrm'], c['zdz'], c['view'], ins['kd'], ins['ks'], lgt, ctx_,
                                                                 bsdf, den_, 1.0)
    R.rnd_seed = 10
    with torch.no_grad():
        a = run(_flags())
        b = run(_flags())
        assert R.rnd_seed == 12 and [s for _, s, _ in seen] == [10, 11] and not torch.equal(a['shaded'], b['shaded'])
        run(_flags(decorrelated=True))
        assert seen[-1][1] is None and R.rnd_seed == 13

        class Plain(torch.nn.Module):                         # the reference's module: forward only
            def forward(self, x):
                return den.forward(x)
        R.rnd_seed = 10
        p = run(_flags(), den_=Plain())
        for k in a:
            assert torch.equal(p[k], a[k]), k
        R.rnd_seed = 10
        raw = run(_flags(), den_=None)
        assert not torch.equal(raw['diffuse_light'], a['diffuse_light'])
        assert torch.equal(raw['shaded'], raw['diffuse_light'] * (ins['kd'] * (1.0 - ins['ks'][..., 2:3])) + raw['specular_light'])
        # one context per frame: frame b is traced against context b in a launch of its own, with the call's seed
        empty = ou.OptiXContext()
        ou.optix_build_bvh(empty, torch.zeros(0, 3, device=dev), torch.zeros(0, 3, dtype=torch.int32, device=dev), rebuild=1)
        del seen[:]
        R.rnd_seed = 10
        two = run(_flags(), ctx_=[ctx, empty], den_=None)
        assert [(s[0] is ctx, s[0] is empty, s[1], s[2][0]) for s in seen] == [(True, False, 10, 1), (False, True, 10, 1)] and R.rnd_seed == 11
        R.rnd_seed = 10
        open_sky = run(_flags(), ctx_=[empty, empty], den_=None)
        R.rnd_seed = 10
        shadowed = run(_flags(), ctx_=[ctx, ctx], den_=None)
        assert tuple(two['shaded'].shape) == (2, 9, 13, 3)
        for k in two:
            assert torch.equal(two[k][:1], shadowed[k][:1]) and torch.equal(two[k][1:], open_sky[k][1:]), k
        assert not torch.equal(shadowed['diffuse_light'][1:], open_sky['diffuse_light'][1:]), 'the occluder shadows nothing in frame 1'
        for bad in (dict(bsdf='kd'), dict(ctx_=None), dict(ctx_=[ctx, ctx, ctx])):
            with pytest.raises(RuntimeError):
                run(_flags(), **bad)
        with pytest.raises(RuntimeError):
            R.shade_lit(_flags(), c['mask'], c['ro'], ins['pos'], ins['nrm'], c['zdz'], c['view'], ins['kd'], ins['ks'], None, ctx, 'pbr', den, 1.0)


# ---- render_mesh -----------------------------------------------------------------------------------------------------------------------------
RES = (48, 40)


class StubTexture(torch.nn.Module):
    """material['kd_ks']: a smooth function of position with two parameters"""

    def __init__(self, dev):
        super().__init__()
        gen = torch.Generator().manual_seed(3)
        self.A = torch.nn.Parameter((torch.randn(3, 6, generator=gen) * 0.6).to(dev))
        self.b = torch.nn.Parameter(torch.tensor([0.3, -0.2, 0.1, -1.0, 0.2, 0.0]).to(dev))

    def sample(self, pos, idx=None, mask=None):
        return torch.sigmoid(pos @ self.A + self.b)


def _scene(dev, grad=False):
    from render import mesh as M, util
    verts, tris = OC.scene_mesh()
    v = np.stack([verts, verts])
    v[1, 4:, 0] += 0.7                                       # frame 1: the occluder has moved
    v[1, 4:, 1] += 0.2
    v_pos = _to(dev, v, grad)
    tex = StubTexture(dev)
    mat = {'kd_ks': tex, 'bsdf': 'pbr'}
    f = _to(dev, tris.astype(np.int64))
    m = M.auto_normals(M.Mesh(v_pos, f, material=mat))
    m_orig = M.auto_normals(M.Mesh(_to(dev, verts), f, material=mat))
    eye = torch.tensor([0.0, 3.0, 4.0])
    mv = util.lookAt(eye, torch.zeros(3), torch.tensor([0.0, 1.0, 0.0]))
    mvp = (util.perspective(0.9, RES[1] / RES[0], 0.1, 100.0) @ mv)[None].repeat(2, 1, 1).to(dev)
    campos = eye[None].repeat(2, 1).to(dev)
    gen = torch.Generator().manual_seed(17)
    B, H, W = 2, RES[0], RES[1]
    draws = {'noise': torch.randn(B, H, W, 3, generator=gen), 'offset': torch.randn(B, H, W, 2, generator=gen) * 0.005,
             'pos_noise': torch.randn(B, H, W, 3, generator=gen) * 0.01}
    bg = torch.rand(B, H, W, 3, generator=gen).to(dev)
    return dict(mesh=m, orig=m_orig, mvp=mvp, campos=campos, draws=draws, bg=bg, v_pos=v_pos, tris=f, tex=tex)


def _lit_kit(dev):
    from render import light
    from denoiser.denoiser import BilateralDenoiser
    import render.optixutils as ou
    fx = OC.shade_fixture(N_SHADE)
    return light.EnvironmentLight(_to(dev, fx['light'], True)), ou.OptiXContext(), BilateralDenoiser(influence=0.5)


def _render(sc, FLAGS, lgt=None, ctx=None, den=None, **kw):
    from render import render as R
    import render.optixutils as ou
    if ctx is not None:
        ou.optix_build_bvh(ctx, sc['mesh'].v_pos, sc['mesh'].t_pos_idx, rebuild=1)          # what geometry.hmsdf records before it renders
    return R.render_mesh(FLAGS, 0, None, sc['mesh'], sc['orig'], sc['mvp'], sc['campos'], lgt, list(RES), spp=1, msaa=True, background=sc['bg'],
                         optix_ctx=ctx, denoiser=den, shadow_scale=1.0, use_uv=False, _rng_draws=sc['draws'], **kw)


def check_render_mesh_unlit_is_untouched(dev):
    """flag absent or false, given a light, a context and a denoiser: bit for bit the render without them; the BVH is never built"""
    from d3h import raytrace as RT
    sc = _scene(dev)
    with torch.no_grad():
        plain = _render(sc, None)
        for F in (None, _flags(), _flags(lit_shading=False)):
            lgt, ctx, den = _lit_kit(dev)
            builds = RT.BUILDS
            out = _render(sc, F, lgt, ctx, den, bsdf='pbr')
            assert RT.BUILDS == builds and ctx.bvh is None
            assert sorted(out) == sorted(plain) and 'diffuse_light' not in out and 'specular_light' not in out
            for k, v in plain.items():
                if torch.is_tensor(v):
                    assert torch.equal(out[k], v), k


def check_render_mesh_lit(dev, monkeypatch):
    from render import render as R, renderutils as ru
    from d3h import imgops as _I, raytrace as RT
    import nvdiffrast.torch as dr
    sc = _scene(dev, grad=True)
    lgt, ctx, den = _lit_kit(dev)
    F = _flags(lit_shading=True)
    calls = []
    real = R.shade_lit

    def spy(*a, **kw):
        out = real(*a, **kw)
        calls.append((a, kw, out))
        return out
    monkeypatch.setattr(R, 'shade_lit', spy)
    recorded = []
    real_record = R.ou.optix_build_bvh

    def record_spy(c, verts, tris, rebuild):
        recorded.append((c, verts, tris))
        return real_record(c, verts, tris, rebuild)
    monkeypatch.setattr(R.ou, 'optix_build_bvh', record_spy)
    names = list(R.ALL_BUFFERS) + list(R.LIT_BUFFERS) + ['_rast']
    builds = RT.BUILDS
    R.rnd_seed = SEED0
    out = _render(sc, F, lgt, ctx, den, buffers=names)
    assert len(calls) == 1 and R.rnd_seed == SEED0 + 1
    a, kw, layer = calls[0]
    # frame 1 was traced against frame 1's mesh: a context per frame, each recorded with that frame's vertices ...
    ctxs = a[10]
    assert isinstance(ctxs, list) and len(ctxs) == 2 and RT.BUILDS == builds + 2 and ctx.bvh is None
    v_all = sc['v_pos'].detach()
    assert not torch.equal(v_all[0], v_all[1])
    assert [r[0] for r in recorded] == [ctx, ctxs[0], ctxs[1]] and recorded[0][1] is sc['mesh'].v_pos
    for b, c in enumerate(ctxs):
        assert c.bvh is not None and c.bvh.F == 4
        assert tuple(recorded[1 + b][1].shape) == (8, 3) and torch.equal(recorded[1 + b][1].detach(), v_all[b]), f'frame {b} was not given its own vertices'
        assert torch.equal(recorded[1 + b][2].long(), sc['tris'])
    # ... and each frame's lit images are those of a one-frame shade against a BVH of that frame's mesh alone, with the same seed and inputs; frame 1
    # against frame 0's mesh (what flattening the batch would trace) gives another image
    with torch.no_grad():
        one = lambda t, b: t[b:b + 1].detach() if torch.is_tensor(t) else t

        def alone_against(b, v):
            c = R.ou.OptiXContext()
            real_record(c, v, sc['tris'].int(), 1)
            R.rnd_seed = SEED0
            return real(a[0], *(one(t, b) for t in a[1:9]), a[9], c, *a[11:])
        for b in range(2):
            own = alone_against(b, v_all[b])
            for k in own:
                assert torch.equal(own[k], layer[k][b:b + 1].detach()), (b, k, float((own[k] - layer[k][b:b + 1].detach()).abs().max()))
        other = alone_against(1, v_all[0])
        assert not torch.equal(other['diffuse_light'], layer['diffuse_light'][1:].detach()), 'frame 1 looks the same under frame 0\'s occluder'
        R.rnd_seed = SEED0 + 1
    # the contexts stay with the record they were made from: a second render against it builds nothing; a new record drops them
    assert ctx.frames is not None and ctx.frames[1] is ctxs and R._frame_contexts(ctx, 2) is ctxs and RT.BUILDS == builds + 5
    del recorded[:]
    assert a[11] == 'pbr' and a[12] is den and tuple(a[1].shape[:3]) == (2, *RES)
    assert torch.equal(a[2], a[3] + a[4] * 0.001)                                       # ro = gb_pos + 0.001 n
    rast = out['_rast']
    cover = rast[..., 3] > 0
    assert torch.equal(a[1][..., 0] > 0, cover) and 0.2 < float(cover.float().mean()) < 0.9
    clip = ru.xfm_points(sc['v_pos'].detach(), sc['mvp'])
    tri = sc['mesh'].t_pos_idx32
    for k, kind, bg in (('shaded', _I.COMP_IMAGE, sc['bg']), ('diffuse_light', _I.COMP_ZERO, None), ('specular_light', _I.COMP_ZERO, None)):
        with torch.no_grad():
            ref = dr.antialias(_I.composite(rast, [(layer[k].detach(), kind, bg)]), rast, clip, tri)
        assert tuple(out[k].shape) == (2, *RES, 4) and torch.isfinite(out[k]).all()
        assert torch.equal(out[k].detach(), ref), (k, float((out[k].detach() - ref).abs().max()))
    # pixels with no covered neighbour: the background, and no light
    far = torch.nn.functional.max_pool2d(cover.float()[:, None], 3, 1, 1)[:, 0] == 0
    assert int(far.sum()) > 50
    assert torch.equal(out['shaded'][..., :3][far], sc['bg'][far]) and (out['shaded'][..., 3][far] == 0).all()
    assert (out['diffuse_light'][far] == 0).all() and (out['specular_light'][far] == 0).all()
    assert float(out['diffuse_light'].detach()[..., :3][cover].min()) >= 0 and float(out['specular_light'].detach()[..., :3].abs().max()) > 0
    # the occluder's shadow moves with the occluder: the ground's light differs between the frames
    assert not torch.equal(out['diffuse_light'][0], out['diffuse_light'][1])
    wgt = torch.rand(out['shaded'].shape, generator=torch.Generator().manual_seed(2)).to(dev)
    ((out['shaded'] * wgt).sum() + out['diffuse_light'].sum() + out['specular_light'].sum()).backward()
    for what, g in (('light', lgt.base.grad), ('A', sc['tex'].A.grad), ('b', sc['tex'].b.grad), ('v_pos', sc['v_pos'].grad)):
        assert g is not None and torch.isfinite(g).all() and float(g.abs().max()) > 0, what
    # 'shaded' alone: the render produces what the lit colour is made of, and the same image
    lit_full = out['shaded'].detach()
    with torch.no_grad():
        R.rnd_seed = SEED0
        alone = _render(sc, F, lgt, ctx, den, buffers=['shaded'])
        assert torch.equal(alone['shaded'], lit_full)
        assert recorded[0][0] is ctx and ctx.frames is not None and ctx.frames[1] is not ctxs and ctx.frames[0] is ctx.pending          # re-recorded: built anew
        assert not any(k in alone for k in ('diffuse_light', 'normal', 'kd', 'ks', 'z_grad'))
        R.rnd_seed = SEED0
        every = _render(sc, F, lgt, ctx, den, extra_dict={'msdf': torch.linspace(0.2, 0.9, 8).to(dev)})
        assert torch.equal(every['shaded'], lit_full) and torch.equal(every['diffuse_light'], out['diffuse_light'].detach())
        assert set(R.ALL_BUFFERS) | set(R.LIT_BUFFERS) <= set(every)
        # 14 buffers for a pass of 12: the light images are the ones that overflow, every buffer the fused loss pass reads stays in the layout
        assert set(every['_layout']) == set(R.ALL_BUFFERS) | {'msdf_image'} and tuple(every['specular_light'].shape) == (2, *RES, 4)
        # the material's bsdf when the argument is None
        sc['mesh'].material['bsdf'] = 'diffuse'
        R.rnd_seed = SEED0
        _render(sc, F, lgt, ctx, den, buffers=['shaded'])
        assert calls[-1][0][11] == 'diffuse'
        sc['mesh'].material['bsdf'] = 'pbr'


def check_render_mesh_unlit_bsdfs(dev, monkeypatch):
    """'normal', 'tangent', 'ks', 'kd' under the flag (render.py:165-174); an invalid name raises"""
    from render import render as R
    from d3h import raytrace as RT
    sc = _scene(dev)
    lgt, ctx, den = _lit_kit(dev)
    F = _flags(lit_shading=True)
    seen = []
    real = R.shade

    def spy(*a, **kw):
        out = real(*a, **kw)
        seen.append((a, dict(out)))
        return out
    monkeypatch.setattr(R, 'shade', spy)
    builds = RT.BUILDS
    with torch.no_grad():
        for bsdf in ('normal', 'tangent', 'ks', 'kd'):
            out = _render(sc, F, lgt, ctx, den, bsdf=bsdf, buffers=['shaded', 'geometric_normal', '_rast'])
            a, layer = seen[-1]
            gb_normal, gb_tangent = a[7], a[8]
            want = {'normal': lambda: (layer['normal'] + 1.0) * 0.5, 'tangent': lambda: (gb_tangent + 1.0) * 0.5, 'ks': lambda: layer['ks'],
                    'kd': lambda: layer['kd']}[bsdf]()
            assert torch.equal(layer['shaded'], want), bsdf
            assert 'diffuse_light' not in out and sorted(k for k in out if not k.startswith('_')) == ['geometric_normal', 'shaded'], sorted(out)
            if bsdf == 'tangent':
                n = sc['draws']['noise'].to(dev)
                assert torch.equal(gb_tangent, torch.cross(n / n.norm(dim=-1, keepdim=True), gb_normal, dim=-1))
            if bsdf == 'ks':
                assert torch.equal(layer['ks'], sc['tex'].sample(a[5])[..., 3:6])
            ids = out['_rast'][..., 3][:, None]
            inside = ((torch.nn.functional.max_pool2d(ids, 3, 1, 1) == ids) & (-torch.nn.functional.max_pool2d(-ids, 3, 1, 1) == ids) & (ids > 0))[:, 0]
            # one triangle all around: composite and antialias leave the layer as it is, up to the lerp's rounding (values <= 1: 4 ulp of 1)
            err = float((out['shaded'][..., :3][inside] - want[inside]).abs().max())
            print(f'{bsdf}: {int(inside.sum())} interior pixels, shaded differs from the formula by {err:.2e} (bound {4 * 2.0 ** -23:.2e})')
            assert int(inside.sum()) > 100 and err <= 4 * 2.0 ** -23
        assert RT.BUILDS == builds and ctx.bvh is None                      # none of these traces a ray
        with pytest.raises(RuntimeError):
            _render(sc, F, lgt, ctx, den, bsdf='phong')


# ---- ticks -----------------------------------------------------------------------------------------------------------------------------------
def check_tick_init_lit(dev):
    import e2e_cases as E
    from render import light, render as R
    from denoiser.denoiser import BilateralDenoiser
    from d3h import raytrace as RT
    import render.optixutils as ou
    st = E.make_state(n=6, res=32, frames=2, n_samples=96)

    def tick(lit):
        P = E.build_product(dev, st, 12, None)
        lgt = light.EnvironmentLight(_to(dev, OC.shade_fixture(N_SHADE)['light'], True))
        F = P['FLAGS']
        if lit:
            F.lit_shading, F.n_samples, F.decorrelated, F.denoiser_demodulate = True, 1, False, True
        P['material']['bsdf'] = 'pbr'
        R.rnd_seed = SEED0
        builds = RT.BUILDS
        del recorded[:]
        with E.fixed_surface_samples(st['sampled_pts'].to(dev) if st.get('sampled_pts') is not None else None):
            r = P['geometry'].tick_init(P['glctx'], P['target'], lgt, P['material'], P['loss_fn'], st['iteration'], BilateralDenoiser(influence=0.5))
        total = r['img_loss'] + r['reg_loss'] + r['normal_loss'] + r['msk_loss']
        total.backward()
        return {k: float(v.detach()) for k, v in r.items() if torch.is_tensor(v) and v.numel() == 1}, lgt.base.grad, RT.BUILDS - builds, P
    recorded = []
    real_record = ou.optix_build_bvh
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(ou, 'optix_build_bvh', lambda c, verts, tris, rebuild: (recorded.append((c, verts)), real_record(c, verts, tris, rebuild))[1])
        unlit, g0, b0, _ = tick(False)
        assert not recorded
        lit, g1, b1, P = tick(True)
    # the tick records the posed batch, and each frame's BVH is built from that frame's posed vertices
    assert len(recorded) == 3 and recorded[0][0] is P['geometry'].optix_ctx
    posed = recorded[0][1].detach()
    assert posed.dim() == 3 and posed.shape[0] == 2 and not torch.equal(posed[0], posed[1])
    for b in range(2):
        assert recorded[1 + b][0] is P['geometry'].optix_ctx.frames[1][b] and torch.equal(recorded[1 + b][1].detach(), posed[b]), b
    print('unlit', unlit, '\nlit  ', lit)
    assert all(np.isfinite(v) for v in lit.values()), lit
    assert b0 == 0 and g0 is None, 'the unlit tick reached the light'
    assert b1 == 2, 'one BVH per posed frame'
    assert lit['img_loss'] != unlit['img_loss'] and abs(lit['msk_loss'] - unlit['msk_loss']) <= 1e-6 * abs(unlit['msk_loss'])          # same geometry
    assert g1 is not None and torch.isfinite(g1).all() and float(g1.abs().max()) > 0
    assert R.rnd_seed == SEED0 + 1
    tex_g = P['tex'].encoder.params.grad
    assert tex_g is not None and torch.isfinite(tex_g).all() and float(tex_g.abs().max()) > 0
