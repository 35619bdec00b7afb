"""Check functions of the general grid encoding (csrc/gridenc.hip, d3h/gridenc.py, the tinycudann shim, MLPTexture3D with another grid),
shared by tests/test_gridenc_emul.py (host emulation, small sizes) and tests/test_gpu_gridenc.py (MI355X, working sizes).

`ref_encode` is a device-free torch restatement of the contract in the docstring of d3h/gridenc.py.  It forms the position the way the kernel
does, as ONE float32 fma -- `(x.double() * float(np.float32(scale)) + 0.5).float()`: the double product of two float32 is exact, so the one
rounding is the fma's -- takes floor and fraction from that float32 value and does everything after it in float64 (or in `dtype`).  Kernel
and restatement therefore agree on every point's cell and NO point is left out of any comparison.

Tolerances are the project's own for this operation (tests/parity_cases.py:1305-1310, tables drawn from U(-0.5, 0.5)): encoding 1e-5 absolute,
table gradient 5e-5 of max(1, |grad|_max), position gradient 5e-3 of its largest element; the texture as a whole 2e-4 relative (check_texmlp).
"""
import math

import numpy as np
import pytest
import torch

PLS = math.exp(math.log(4096 / 16) / 15)          # render/mlptexture.py:62-65
REF_CFG = {'otype': 'HashGrid', 'n_levels': 5, 'n_features_per_level': 2, 'log2_hashmap_size': 21, 'base_resolution': 16, 'per_level_scale': PLS}
TOL_ENC, TOL_TAB, TOL_X, TOL_TEX = 1e-5, 5e-5, 5e-3, 2e-4
_DEFAULTS = {'n_levels': 16, 'n_features_per_level': 2, 'log2_hashmap_size': 19, 'base_resolution': 16, 'per_level_scale': 2.0, 'interpolation': 'Linear'}


def cfg16(T, **kw):
    """the 16-level grid the reference's per-level scale was computed for (render/mlptexture.py:62-75 with "n_levels": 16)"""
    return dict({'otype': 'HashGrid', 'n_levels': 16, 'n_features_per_level': 2, 'log2_hashmap_size': T, 'base_resolution': 16, 'per_level_scale': PLS}, **kw)


def ref_layout(D, c):
    """section 1 of the contract: [(scale, res, offset, size, hashed)], total entries -- float32 scale, integers exact"""
    g = dict(_DEFAULTS, **c)
    gtype = g.get('type', {'HashGrid': 'Hash', 'DenseGrid': 'Dense', 'Grid': 'Hash'}[g.get('otype', 'HashGrid')])
    out, off = [], 0
    for l in range(g['n_levels']):
        scale = np.float32(np.exp2(np.float32(l) * np.log2(np.float32(g['per_level_scale'])))) * np.float32(g['base_resolution']) - np.float32(1)
        res = int(math.ceil(float(scale))) + 1
        size = (res ** D + 7) // 8 * 8
        if gtype == 'Hash':
            size = min(size, 2 ** g['log2_hashmap_size'])
        out.append((float(scale), res, off, size, res ** D > size))
        off += size
    return out, off


def ref_encode(x, tables, lay, F, interpolation='Linear', dtype=torch.float64):
    """x [N, D] float32; tables: one [size_l * F] tensor per level (separate leaves, so that a gather's gradient is a level's size) -> [N, L * F]"""
    D = x.shape[1]
    feats = []
    for (scale, res, off, size, hashed), tab in zip(lay, tables):
        p = (x.double() * float(np.float32(scale)) + 0.5).float()
        fl = torch.floor(p).detach()
        fr = (p - fl).to(dtype)
        q = fl.long()
        w = fr * fr * (3.0 - 2.0 * fr) if interpolation == 'Smoothstep' else fr
        t2 = tab.to(dtype).view(-1, F)
        acc = 0
        for c in range(2 ** D):
            wc = 1.0
            qs = []
            for d in range(D):
                bit = (c >> d) & 1
                wc = wc * (w[:, d] if bit else (1.0 - w[:, d]))
                qs.append(q[:, d] + bit)
            if hashed:
                idx = qs[0] & 0xFFFFFFFF
                for d, prime in zip(range(1, D), (2654435761, 805459861)):
                    idx = idx ^ ((qs[d] * prime) & 0xFFFFFFFF)
            else:
                idx = sum(qs[d] * res ** d for d in range(D))
            acc = acc + wc[:, None] * t2[idx % size]
        feats.append(acc)
    return torch.cat(feats, -1)


def split_table(table, lay, F):
    return [table[off * F:(off + size) * F] for _, _, off, size, _ in lay]


def make_cfg(D, c):
    """the product's GridConfig with its layout checked against the restatement's: integers identical; the float32 scales within what two
    float32 libraries may differ by (numpy's and libm's log2f 1 ulp each: 2 ulp on l * log2 s, which exp2 turns into a relative
    ln 2 * l * log2 s * 2 ulp, plus 2 ulp for exp2f itself and the product).  The restatement then runs on the library's scales, so that
    both sides place every point in the same cell."""
    from d3h import gridenc
    cfg = gridenc.GridConfig(D, c)
    lay, total = ref_layout(D, c)
    assert cfg.n_entries == total and cfg.n_params == total * cfg.n_features, (cfg.n_entries, total)
    assert [(r, o, s, h) for _, r, o, s, h in lay] == list(zip(cfg.res, cfg.offset, cfg.size, cfg.hashed))
    for l, ((sc, *_), s2) in enumerate(zip(lay, cfg.scale)):
        ulps = 2 + 2 * math.log(2) * l * abs(math.log2(cfg.per_level_scale))
        assert abs(sc - s2) <= 1.2e-7 * ulps * (abs(sc) + 1.0), (l, sc, s2)
    lay = [(s2,) + tuple(rest) for (_, *rest), s2 in zip(lay, cfg.scale)]
    return cfg, lay


def _table(cfg, gen, lo=-0.5, hi=0.5):
    return torch.rand(cfg.n_params, generator=gen) * (hi - lo) + lo


def run_kernel(dev, x, table, cfg, G, grad_x=True, grad_t=True):
    from d3h import gridenc
    xa, ta = x.clone().to(dev).requires_grad_(grad_x), table.clone().to(dev).requires_grad_(grad_t)
    e = gridenc.grid_encode(xa, ta, cfg)
    if grad_x or grad_t:
        (e * G.to(dev)).sum().backward()
    return e.detach(), xa.grad, ta.grad


def run_ref(dev, x, table, lay, F, interpolation, G, dtype=torch.float64):
    """the restatement on `dev` (float64 torch ops; on the GPU box that is the GPU, so that 2^20 points take seconds), one level at a
    time so that only one level's autograd graph is alive"""
    xr = x.clone().to(dev).requires_grad_(True)
    tabs = [t.clone().to(dev).to(dtype).requires_grad_(True) for t in split_table(table, lay, F)]
    Gd = G.to(dev).to(dtype)
    outs = []
    for l in range(len(lay)):
        e = ref_encode(xr, tabs[l:l + 1], lay[l:l + 1], F, interpolation, dtype)
        (e * Gd[:, l * F:(l + 1) * F]).sum().backward()
        outs.append(e.detach())
    return torch.cat(outs, -1), xr.grad, torch.cat([t.grad for t in tabs])


def compare(tag, got, ref, report=None):
    e, dx, dt = got
    er, dxr, dtr = ref
    fig = {'enc_abs': float((e.double() - er.double()).abs().max()) if e.numel() else 0.0}
    if dt is not None:
        fig['tab_abs'], fig['tab_max'] = float((dt.double() - dtr.double()).abs().max()), float(dtr.abs().max())
    if dx is not None and dx.numel():
        fig['x_abs'], fig['x_max'] = float((dx.double() - dxr.double()).abs().max()), float(dxr.abs().max())
    print(f'[gridenc] {tag}: {fig}')
    if report is not None:
        report[tag] = fig
    assert fig['enc_abs'] < TOL_ENC, (tag, fig)
    if 'tab_abs' in fig:
        assert fig['tab_abs'] < TOL_TAB * max(1.0, fig['tab_max']), (tag, fig)
    if 'x_abs' in fig:
        assert fig['x_abs'] < TOL_X * fig['x_max'], (tag, fig)
    return fig


def check_case(dev, D, c, n, seed=0, x=None, tag=None, report=None):
    """value, table gradient and position gradient of one configuration against the restatement; every point takes part"""
    cfg, lay = make_cfg(D, c)
    gen = torch.Generator().manual_seed(seed)
    table = _table(cfg, gen)
    if x is None:
        x = torch.rand(n, D, generator=gen)
    G = torch.randn(x.shape[0], cfg.n_output_dims, generator=gen)
    got = run_kernel(dev, x, table, cfg, G)
    ref = run_ref(dev, x, table, lay, cfg.n_features, cfg.interpolation, G)
    compare(tag or f'D={D} {c}', got, ref, report)
    return cfg, lay, got


# ---- 1. anchor to the existing oracle --------------------------------------------------------------------------------------------------------
def check_anchor(dev, n=5000):
    """gridenc.grid_encode on the reference configuration against oracle/texmlp.py and against the fused kernels' stand-alone encoding, value and
    both gradients, x exactly 0 and exactly 1 (the level-0 wrap) included.  The oracle forms p with a multiply and an add: 1e-5 allows that
    distance (measured 5.1e-6 on the CPU for 5 000 points)."""
    from d3h import texmlp, gridenc
    from oracle import texmlp as OT
    cfg, lay = make_cfg(3, REF_CFG)
    olay, ototal = OT.grid_layout()
    assert ototal == cfg.n_entries == 532792 and cfg.n_params == texmlp.grid_param_count() and not any(cfg.hashed)
    assert [(r, o, s) for _, r, o, s in olay] == list(zip(cfg.res, cfg.offset, cfg.size))
    gen = torch.Generator().manual_seed(3)
    table = _table(cfg, gen)
    x = torch.rand(n, 3, generator=gen)
    x[0], x[1], x[2], x[3] = 0.0, 1.0, torch.tensor([1.0, 0.0, 0.5]), torch.tensor([0.0, 1.0, 1.0])
    G = torch.randn(n, 10, generator=gen)
    got = run_kernel(dev, x, table, cfg, G)
    # the oracle
    xr, tr = x.clone().requires_grad_(True), table.clone().requires_grad_(True)
    er = OT.grid_encode(xr, tr)
    (er * G).sum().backward()
    compare('anchor vs oracle/texmlp.py', tuple(t.cpu() for t in got), (er.detach(), xr.grad, tr.grad))
    # the fused kernels' encoding (the same fma: same cells)
    xa, ta = x.clone().to(dev).requires_grad_(True), table.clone().to(dev).requires_grad_(True)
    ed = texmlp.grid_encode(xa, ta)
    (ed * G.to(dev)).sum().backward()
    compare('anchor vs d3h.texmlp.grid_encode', got, (ed.detach(), xa.grad, ta.grad))
    # and the restatement itself
    compare('anchor vs ref_encode', got, run_ref(dev, x, table, lay, 2, 'Linear', G))


# ---- 2. hashed levels ------------------------------------------------------------------------------------------------------------------------
def check_hashed(dev, T, n, report=None):
    import tinycudann as tcnn
    c = cfg16(T)
    cfg, lay, _ = check_case(dev, 3, c, n, seed=11, tag=f'16 levels T={T} n={n}', report=report)
    assert any(cfg.hashed) and not all(cfg.hashed), cfg.hashed
    enc = tcnn.Encoding(3, c)
    assert enc.params.numel() == 2 * sum(s for _, _, _, s, _ in lay) and enc.n_output_dims == 32
    return cfg


def check_hashed_collisions(dev):
    """T = 14 on 5 000 points: 247 296 entries, levels 2..15 hashed, most of the table touched, so different cells share entries"""
    cfg = check_hashed(dev, 14, 5000)
    assert cfg.n_entries == 247296 and cfg.hashed == [False, False] + [True] * 14


# ---- 3. the matrix ---------------------------------------------------------------------------------------------------------------------------
def matrix_cases():
    out = []
    for D in (2, 3):
        for F in (1, 2, 4, 8):
            for interp in ('Linear', 'Smoothstep'):
                for otype in ('HashGrid', 'DenseGrid'):
                    k = len(out)
                    out.append((D, {'otype': otype, 'n_levels': 3 + k % 3, 'n_features_per_level': F, 'log2_hashmap_size': 9 if D == 3 else 8,
                                    'base_resolution': 4 + k % 5, 'per_level_scale': 2.0 if k % 2 else 1.5, 'interpolation': interp}))
    out.append((3, {'otype': 'Grid', 'type': 'Hash', 'n_levels': 1, 'n_features_per_level': 2, 'log2_hashmap_size': 6, 'base_resolution': 9}))
    out.append((2, {'otype': 'Grid', 'type': 'Dense', 'n_levels': 1, 'n_features_per_level': 4, 'base_resolution': 7, 'interpolation': 'Smoothstep'}))
    return out


def check_matrix(dev, n):
    from d3h import gridenc
    n_hashed = 0
    for k, (D, c) in enumerate(matrix_cases()):
        cfg, _, _ = check_case(dev, D, c, n + 13 * k, seed=100 + k)
        dense = c.get('otype') == 'DenseGrid' or c.get('type') == 'Dense'
        if dense:
            assert not any(cfg.hashed), (c, cfg)
        n_hashed += any(cfg.hashed)
    assert n_hashed >= 8
    # a DenseGrid whose res^D exceeds 2^T stays unhashed (and keeps its full size)
    cfg = gridenc.GridConfig(3, {'otype': 'DenseGrid', 'n_levels': 2, 'log2_hashmap_size': 4, 'base_resolution': 8})
    assert cfg.size == [512, 4096] and cfg.hashed == [False, False]
    # defaults of absent keys
    cfg = gridenc.GridConfig(3, {'otype': 'HashGrid'})
    assert (cfg.n_levels, cfg.n_features, cfg.log2_hashmap_size, cfg.base_resolution, cfg.per_level_scale, cfg.interpolation) == (16, 2, 19, 16, 2.0, 'Linear')


# ---- 4. accumulation -------------------------------------------------------------------------------------------------------------------------
def coherent_curve(m):
    """the spatially coherent curve of check_texmlp (tests/parity_cases.py:1311-1326): consecutive points in the same or a neighbouring cell"""
    t_ = torch.arange(m, dtype=torch.float32) / m
    xc = torch.stack([0.1 + 0.8 * t_, 0.5 + 0.3 * torch.sin(9.0 * t_), 0.5 + 0.25 * torch.cos(5.0 * t_)], -1)
    xc[m // 2:] = xc[m // 2:].flip(0)[:, [1, 2, 0]]
    return xc


def check_accumulation(dev, T, m, n_same):
    cfg, lay, got = check_case(dev, 3, cfg16(T), 0, seed=21, x=coherent_curve(m), tag=f'coherent curve m={m} T={T}')
    assert float(got[2].abs().max()) > 3.0                     # many points per coarse entry: the sums are not single contributions
    # every point identical: every lane of every wave on the same 8 entries of each level
    x = torch.tensor([[0.3137, 0.7071, 0.5523]]).repeat(n_same, 1)
    _, _, got = check_case(dev, 3, cfg16(T), 0, seed=22, x=x, tag=f'{n_same} identical points T={T}')
    assert int((got[2] != 0).sum()) <= 8 * 16 * 2


# ---- 5. edges --------------------------------------------------------------------------------------------------------------------------------
def check_edges(dev, T=14, n_big=777):
    from d3h import gridenc
    c = cfg16(T)
    cfg, lay = make_cfg(3, c)
    gen = torch.Generator().manual_seed(31)
    table = _table(cfg, gen)
    # N = 0: empty tensors, no launch
    x0 = torch.zeros(0, 3).to(dev).requires_grad_(True)
    t0 = table.clone().to(dev).requires_grad_(True)
    e0 = gridenc.grid_encode(x0, t0, cfg)
    assert e0.shape == (0, 32) and e0.dtype == torch.float32
    e0.sum().backward()
    assert x0.grad.shape == (0, 3) and t0.grad.shape == t0.shape and float(t0.grad.abs().max()) == 0.0
    for n in (1, n_big):                                       # N = 1; N not a multiple of 64
        check_case(dev, 3, c, n, seed=32 + n, tag=f'N={n}')
    # gradient for the table only, for x only, for neither
    x = torch.rand(300, 3, generator=gen)
    G = torch.randn(300, 32, generator=gen)
    ref = run_ref(dev, x, table, lay, 2, 'Linear', G)
    for gx, gt in ((False, True), (True, False), (False, False)):
        e, dx, dt = run_kernel(dev, x, table, cfg, G, grad_x=gx, grad_t=gt)
        assert (dx is not None) == gx and (dt is not None) == gt
        compare(f'grad_x={gx} grad_t={gt}', (e, dx, dt), ref)


def check_out_of_range(dev, nonfinite, n=600, T=14):
    """rows outside [0, 1] (up to +-1e9; on the emulator also inf / nan) mixed into a batch: the call returns, and the in-range rows of the
    output are bit-identical to a batch without the others, their position gradient within the usual distance of the restatement"""
    from d3h import gridenc
    for D, c in ((3, cfg16(T)), (2, {'otype': 'HashGrid', 'n_levels': 8, 'n_features_per_level': 4, 'log2_hashmap_size': 10, 'base_resolution': 8,
                                      'per_level_scale': 1.7, 'interpolation': 'Smoothstep'}),
                 (3, {'otype': 'DenseGrid', 'n_levels': 3, 'n_features_per_level': 1, 'base_resolution': 5})):
        cfg, lay = make_cfg(D, c)
        gen = torch.Generator().manual_seed(41)
        table = _table(cfg, gen)
        x = torch.rand(n, D, generator=gen)
        bad = torch.tensor([-1e9, 1e9, -3.5, 2.25, -1e-3, 1.0 + 1e-3, 4e6, -7e4, 3e38, -3e38] + ([float('inf'), -float('inf'), float('nan')] if nonfinite else []))
        rows = torch.arange(0, n, 7)
        xm = x.clone()
        for j, r in enumerate(rows.tolist()):
            xm[r, j % D] = bad[j % len(bad)]
            if j % 3 == 0:
                xm[r, (j + 1) % D] = bad[(j + 5) % len(bad)]
        keep = torch.ones(n, dtype=torch.bool)
        keep[rows] = False
        G = torch.randn(n, cfg.n_output_dims, generator=gen)
        G[~keep] = 0.25
        e, dx, dt = run_kernel(dev, xm, table, cfg, G)
        assert e.shape == (n, cfg.n_output_dims) and dt.shape == table.shape
        e_in, _, _ = run_kernel(dev, x[keep], table, cfg, G[keep], grad_x=False, grad_t=False)
        assert torch.equal(e[keep.to(e.device)], e_in)
        er, dxr, _ = run_ref(dev, x[keep], table, lay, cfg.n_features, cfg.interpolation, G[keep])
        k = keep.to(e.device)
        compare(f'in-range rows of a mixed batch D={D}', (e[k], dx[k], None), (er, dxr, None))


# ---- 6. validation before any launch -----------------------------------------------------------------------------------------------------------
def check_validation(dev):
    from d3h import gridenc
    import tinycudann as tcnn
    H = {'otype': 'HashGrid'}
    for mk in (gridenc.GridConfig, tcnn.Encoding):
        for D, c, err, key in ((1, H, NotImplementedError, 'n_input_dims'), (4, H, NotImplementedError, 'n_input_dims'),
                               (3, dict(H, n_features_per_level=3), NotImplementedError, 'n_features_per_level'),
                               (3, dict(H, n_features_per_level=16), NotImplementedError, 'n_features_per_level'),
                               (3, {'otype': 'Grid', 'type': 'Tiled'}, NotImplementedError, 'type'),
                               (3, {'otype': 'TiledGrid'}, NotImplementedError, 'type'),
                               (3, dict(H, interpolation='Nearest'), NotImplementedError, 'interpolation'),
                               (3, {'otype': 'Frequency'}, NotImplementedError, 'otype'),
                               (3, {'otype': 'SphericalHarmonics'}, NotImplementedError, 'otype'),
                               (3, dict(H, n_levels=0), ValueError, 'n_levels'), (3, dict(H, n_levels=-2), ValueError, 'n_levels'),
                               (3, dict(H, base_resolution=0), ValueError, 'base_resolution'),
                               (3, dict(H, per_level_scale=0.0), ValueError, 'per_level_scale'),
                               (3, dict(H, per_level_scale=-1.5), ValueError, 'per_level_scale'),
                               (3, {'otype': 'DenseGrid', 'n_levels': 8, 'base_resolution': 512}, ValueError, '2\\^31 entries'),
                               (3, dict(H, log2_hashmap_size=31, n_levels=16, base_resolution=2048), ValueError, '2\\^31 entries'),
                               (2, {'otype': 'DenseGrid', 'n_levels': 2, 'base_resolution': 40000}, ValueError, '2\\^31 entries')):
            with pytest.raises(err, match=key):
                mk(D, c)
    cfg = gridenc.GridConfig(3, dict(H, n_levels=2, log2_hashmap_size=8))
    good_x, good_t = torch.rand(5, 3).to(dev), torch.zeros(cfg.n_params).to(dev)
    with pytest.raises(ValueError, match='columns'):
        gridenc.grid_encode(torch.rand(5, 2).to(dev), good_t, cfg)
    with pytest.raises(ValueError, match='floats'):
        gridenc.grid_encode(good_x, torch.zeros(cfg.n_params - 2).to(dev), cfg)
    e = gridenc.grid_encode(good_x, good_t.requires_grad_(True), cfg)
    with pytest.raises(RuntimeError, match='once_differentiable|differentiated twice|double backward'):       # first order only
        (gt,) = torch.autograd.grad((e * e).sum(), good_t, create_graph=True)     # (the incoming gradient 2 e carries a graph)
        gt.sum().backward()


# ---- 7. shim and texture ----------------------------------------------------------------------------------------------------------------------
def check_shim(dev, monkeypatch):
    import tinycudann as tcnn
    from d3h import texmlp, gridenc
    from render.mlptexture import MLPTexture3D
    c = {'otype': 'HashGrid', 'n_levels': 6, 'n_features_per_level': 4, 'log2_hashmap_size': 10, 'base_resolution': 8, 'per_level_scale': 1.6}
    torch.manual_seed(99)                 # the features come from `seed`, not from the global generator
    a = tcnn.Encoding(3, c).to(dev)
    b = tcnn.Encoding(3, c, seed=1337).to(dev)
    other = tcnn.Encoding(3, c, seed=7).to(dev)
    assert a.n_input_dims == 3 and a.n_output_dims == 24 and a.params.dtype == torch.float32 and a.params.numel() == a.cfg.n_params
    assert torch.equal(a.params, b.params) and not torch.equal(a.params, other.params)
    assert float(a.params.detach().abs().max()) <= 1e-4 and float(a.params.detach().abs().max()) > 0.9e-4 and float(a.params.detach().min()) < 0 < float(a.params.detach().max())
    x = torch.rand(50, 3).to(dev)
    y = a(x)
    assert y.shape == (50, 24) and y.dtype == torch.float32
    assert torch.equal(y, gridenc.grid_encode(x, a.params, a.cfg))
    y.sum().backward()
    assert a.params.grad is not None and a.params.grad.shape == a.params.shape
    e2 = tcnn.Encoding(2, {'otype': 'DenseGrid', 'n_levels': 3, 'n_features_per_level': 8, 'base_resolution': 4}).to(dev)
    assert e2(torch.rand(9, 2).to(dev)).shape == (9, 24)
    # the reference configuration stays on the fused kernels' encoding
    calls = {'enc': 0, 'tex': 0, 'gen': 0}
    real_enc, real_tex, real_gen = texmlp.grid_encode, texmlp.texture_mlp, gridenc.grid_encode
    monkeypatch.setattr(texmlp, 'grid_encode', lambda *a_, **k: (calls.__setitem__('enc', calls['enc'] + 1), real_enc(*a_, **k))[1])
    monkeypatch.setattr(texmlp, 'texture_mlp', lambda *a_, **k: (calls.__setitem__('tex', calls['tex'] + 1), real_tex(*a_, **k))[1])
    monkeypatch.setattr(gridenc, 'grid_encode', lambda *a_, **k: (calls.__setitem__('gen', calls['gen'] + 1), real_gen(*a_, **k))[1])
    r = tcnn.Encoding(3, REF_CFG).to(dev)
    assert r.cfg is None and r.params.numel() == texmlp.grid_param_count() and r.n_output_dims == 10
    assert r(x).shape == (50, 10) and calls == {'enc': 1, 'tex': 0, 'gen': 0}
    mm = [torch.zeros(6).to(dev), torch.ones(6).to(dev)]
    tex = MLPTexture3D(None, channels=6, min_max=mm).to(dev)
    assert tex.fused and tex.encoder.cfg is None and sorted(tex.state_dict()) == ['encoder.params', 'net.net.0.weight', 'net.net.2.weight', 'net.net.4.weight']
    assert tex.sample(torch.rand(4, 5, 3).to(dev) - 0.5).shape == (4, 5, 6) and calls == {'enc': 1, 'tex': 1, 'gen': 0}
    gen_tex = MLPTexture3D(None, channels=6, min_max=mm, enc_cfg=c).to(dev)
    assert not gen_tex.fused and sorted(gen_tex.state_dict()) == sorted(tex.state_dict())
    assert gen_tex.sample(torch.rand(4, 5, 3).to(dev) - 0.5).shape == (4, 5, 6) and calls == {'enc': 1, 'tex': 1, 'gen': 1}


class _ScaleGrad(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, s):
        ctx.s = s
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return g * ctx.s, None


def check_texture(dev, n, enc_cfg=None, **shape):
    """MLPTexture3D on the composed path against a float64 restatement of the reference's sample() (render/mlptexture.py:91-107) built on
    ref_encode: value, every parameter gradient and the position gradient, 2e-4 relative (check_texmlp's figure), with a mask.
    The state is kink-free (Scene.set_kinkfree_texture's construction: positive features and positive hidden weights keep every hidden
    pre-activation positive), so float32 and float64 evaluate the bias-free ReLU network inside one linear piece; the box normalisation is
    done in float32 with the same torch ops on both sides, so both hand the encoding the same float32 coordinates."""
    from render.mlptexture import MLPTexture3D
    gen = torch.Generator().manual_seed(51)
    C = shape.get('channels', 6)
    lo, hi = torch.rand(C, generator=gen) * 0.1, 0.5 + torch.rand(C, generator=gen)
    tex = MLPTexture3D(None, min_max=[lo.to(dev), hi.to(dev)], enc_cfg=enc_cfg, **dict({'channels': 6}, **shape)).to(dev)
    assert not tex.fused
    cfg, lay = make_cfg(3, enc_cfg if enc_cfg is not None else REF_CFG)        # (the default grid: the encoder is the fused kernels' own, cfg None)
    lins = [m for m in tex.net.net if isinstance(m, torch.nn.Linear)]
    assert len(lins) == shape.get('hidden', 2) + 1 and lins[0].weight.shape == (shape.get('internal_dims', 32), cfg.n_output_dims) and lins[-1].weight.shape[0] == C
    with torch.no_grad():
        tex.encoder.params.copy_((torch.rand(cfg.n_params, generator=gen) * 0.30 + 0.05).to(dev))
        for m in lins[:-1]:
            m.weight.copy_(((torch.rand(m.weight.shape, generator=gen) + 0.05) / m.weight.shape[1]).to(dev))
        lins[-1].weight.copy_(((torch.rand(lins[-1].weight.shape, generator=gen) * 2 - 1) / lins[-1].weight.shape[1] ** 0.5).to(dev))
    texc = (torch.rand(n, 3, generator=gen) * torch.tensor([1.8, 2.2, 0.6]) + torch.tensor([-1.0, -1.4, -0.3])).to(dev)     # partly outside the box
    texc[0] = torch.tensor([-0.8, -1.2, -0.2])                                   # exactly on the x_n == 1 corner
    mask = (torch.rand(n, generator=gen) > 0.2).float().to(dev)
    G = torch.randn(n, C, generator=gen).to(dev)
    xa = texc.clone().requires_grad_(True)
    out = tex.sample(xa.reshape(n // 4, 4, 3), None, mask=mask.reshape(n // 4, 4))
    assert out.shape == (n // 4, 4, C) and out.dtype == torch.float32
    (out.reshape(n, C) * G).sum().backward()
    assert float(out.reshape(n, C)[mask <= 0].abs().max()) == 0.0 and float(xa.grad[mask <= 0].abs().max()) == 0.0
    # the restatement
    xr = texc.clone().requires_grad_(True)
    b0, b1 = torch.tensor(tex.BBOX[:3], device=dev), torch.tensor(tex.BBOX[3:], device=dev)
    xn = torch.clamp((xr - b0[None]) / (b1 - b0)[None], min=0, max=1)
    tabs = [t.detach().clone().double().requires_grad_(True) for t in split_table(tex.encoder.params, lay, cfg.n_features)]
    ws = [m.weight.detach().clone().double().requires_grad_(True) for m in lins]
    h = _ScaleGrad.apply(ref_encode(xn, tabs, lay, cfg.n_features, cfg.interpolation), 128.0)
    for w in ws[:-1]:
        h = torch.relu(h @ w.t())
        assert float(h.min()) > 0.0                                              # kink-free: no unit sits at its kink
    o = torch.sigmoid(h @ ws[-1].t()) * (hi - lo).double().to(dev)[None] + lo.double().to(dev)[None]
    o = o * (mask > 0).double()[:, None]
    (o * G.double()).sum().backward()
    rel = lambda a, b: float((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-30))
    fig = {'out': rel(out.reshape(n, C), o.detach()), 'x': rel(xa.grad, xr.grad), 'table': rel(tex.encoder.params.grad, torch.cat([t.grad for t in tabs]))}
    for k, (m, w) in enumerate(zip(lins, ws)):
        fig[f'w{k}'] = rel(m.weight.grad, w.grad)
    print(f'[gridenc] texture {enc_cfg} {shape}: {fig}')
    assert all(v < TOL_TEX for v in fig.values()), fig
    assert float(xr.grad.abs().max()) > 0 and float(tabs[0].grad.abs().max()) > 0


# ---- 8. a step -------------------------------------------------------------------------------------------------------------------------------
def check_step(dev, monkeypatch, T=19, res=128, grid_n=12, body_verts=2048):
    """one tick_init step of the synthetic scene whose texture is the 16-level grid, under the fused optimiser and under the torch ones"""
    from d3h import scene as S
    ell = lambda x: (((x - torch.tensor([0.0, -0.4, 0.0], device=x.device)) / torch.tensor([0.55, 0.8, 0.45], device=x.device)).norm(dim=-1) - 1.0) * 0.4
    for fused in (True, False):
        monkeypatch.setattr(S, 'FUSED_OPTIMIZER', fused)
        torch.manual_seed(0)
        sc = S.Scene(res=res, grid_n=grid_n, n_frames=2, device=dev, prefit_steps=150, loss_set='full', body_verts=body_verts, sdf_fn=ell,
                     tex_enc_cfg=cfg16(T))
        tex = sc.material['kd_ks']
        enc = tex.encoder.params
        assert not tex.fused and enc.numel() == tex.encoder.cfg.n_params and any(tex.encoder.cfg.hashed)
        assert (sc.opt is not None) == fused and any(p is enc for grp in (sc.opt or sc.opt_mat).param_groups for p in grp['params'])
        bg = torch.rand(2, res, res, 3, device=dev)
        sc._zero_grad()
        r = sc.geometry.tick_init(sc.glctx, sc.target(bg), None, sc.material, sc.loss_fn, 5, None)
        total = r['d3h_total'] if 'd3h_total' in r else (r['msk_loss'] + r['reg_loss'] + r['normal_loss'] + r.get('ssim_loss', 0.0))
        total.backward()
        losses = {k: float(v.detach()) for k, v in r.items() if torch.is_tensor(v) and v.numel() == 1}
        assert all(np.isfinite(v) for v in losses.values()), losses
        assert enc.grad is not None and bool(torch.isfinite(enc.grad).all()) and float(enc.grad.abs().max()) > 0
        assert all(m.weight.grad is not None and bool(torch.isfinite(m.weight.grad).all()) for m in tex.net.net if isinstance(m, torch.nn.Linear))
        before = enc.detach().clone()
        sc._optimizer_step()
        # the reference's schedule (train.py:573-576) is a linear warm-up FROM ZERO: the step of iteration 0 runs at learning rate 0 and
        # only advances the moments and the schedule; the next step, at 1 / 300 of the rate, is the first that moves a parameter
        lrs = [grp['lr'] for grp in (sc.opt or sc.opt_mat).param_groups if any(p is enc for p in grp['params'])]
        print(f'[gridenc] step fused={fused}: losses {losses}, |enc.grad|_max {float(enc.grad.abs().max()):.3e}, lr after the first step {lrs}')
        assert lrs and lrs[0] > 0
        sc._optimizer_step()
        assert not torch.equal(before, enc.detach()) and bool(torch.isfinite(enc).all())
