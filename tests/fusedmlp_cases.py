"""Check functions of the general fused MLP (csrc/fusedmlp.hip, d3h/fusedmlp.py, tinycudann.Network / NetworkWithInputEncoding, the
`fused_net` routing of MLPTexture3D), shared by tests/test_fusedmlp_emul.py (host emulation) and tests/test_gpu_fusedmlp.py (MI355X).

`ref_mlp` is a float64 torch restatement of the contract in the docstring of d3h/fusedmlp.py: h = act(h @ W.T) per layer, the mask, the
affine output map and the input-gradient scale.  The bar is the project's own for the texture network, TOL_TEX = 2e-4 of
tests/gridenc_cases.py (check_texmlp's figure): maximum absolute difference over the reference's maximum magnitude, per tensor.  A kernel
that is an fmaf chain sits near 1e-7 -- 1e-6 there; an indexing, padding or activation-mask error is O(1).

Kinks.  The states are general (Xavier weights, inputs in [-1, 1]), so ReLU units do switch off.  A unit whose float64 pre-activation is
within 1e-5 of its layer's largest magnitude of zero could be on the other side in float32, which would change the gradient of that row by
O(1) without being an error: before the kernel runs, the rows of the upstream gradient G with such a unit are zeroed (their VALUES are
still compared) and the check asserts that at most 10 % of the rows are dropped.  The smooth activations need no exclusion.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from gridenc_cases import TOL_TEX, REF_CFG, cfg16

ACT = {'None': lambda z: z, 'ReLU': torch.relu, 'LeakyReLU': lambda z: F.leaky_relu(z, 0.01), 'Sigmoid': torch.sigmoid, 'Tanh': torch.tanh,
       'Softplus': F.softplus, 'Exponential': torch.exp}
KINKED = ('ReLU', 'LeakyReLU')
SHAPES = [(3, 16, 1, 1), (7, 32, 2, 3), (32, 32, 2, 6), (32, 64, 3, 9), (20, 128, 8, 16)]
SHAPE_GPU_ONLY = (256, 128, 2, 128)


class _ScaleGrad(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, s):
        ctx.s = s
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return g * ctx.s, None


def net_cfg(shape, act='ReLU', out_act='None'):
    n_in, w, hidden, n_out = shape
    return n_in, n_out, {'otype': 'FullyFusedMLP', 'activation': act, 'output_activation': out_act, 'n_neurons': w, 'n_hidden_layers': hidden}


def make_state(cfg, n, seed, mask_frac=0.0, affine=False):
    """Xavier-uniform matrices, x in [-1, 1], a random upstream gradient; optionally a mask with about `mask_frac` zeros and an affine map"""
    g = torch.Generator().manual_seed(seed)
    ws = [(torch.rand(fo, fi, generator=g) * 2 - 1) * (6.0 / (fi + fo)) ** 0.5 for fo, fi in cfg.shapes]
    x = torch.rand(n, cfg.n_input_dims, generator=g) * 2 - 1
    G = torch.randn(n, cfg.n_output_dims, generator=g)
    mask = (torch.rand(n, generator=g) > mask_frac).float() if mask_frac > 0 else None
    scale = (0.5 + torch.rand(cfg.n_output_dims, generator=g)) if affine else None
    bias = (torch.rand(cfg.n_output_dims, generator=g) - 0.5) if affine else None
    return x, ws, G, mask, scale, bias


def ref_mlp(x, ws, cfg, mask=None, scale=None, bias=None, in_grad_scale=1.0, pre=None):
    """the float64 restatement; `pre` collects the pre-activations in front of a kinked activation"""
    h = _ScaleGrad.apply(x.double(), in_grad_scale) if in_grad_scale != 1.0 else x.double()
    for w in ws[:-1]:
        z = h @ w.double().t()
        if pre is not None and cfg.activation in KINKED:
            pre.append(z.detach())
        h = ACT[cfg.activation](z)
    z = h @ ws[-1].double().t()
    if pre is not None and cfg.output_activation in KINKED:
        pre.append(z.detach())                             # (a kinked OUTPUT activation: its pre-activation counts as well)
    o = ACT[cfg.output_activation](z)
    if scale is not None:
        o = o * scale.double()[None]
    if bias is not None:
        o = o + bias.double()[None]
    if mask is not None:
        o = o * (mask > 0).double()[:, None]
    return o


def drop_kinks(G, pre, tag):
    """zero the rows of G in which one of the pre-activations `pre` (those in front of a ReLU or LeakyReLU) is within 1e-5 of its layer's
    largest magnitude of zero (module docstring)"""
    if G.shape[0] == 0:
        return G, 0.0
    near = torch.zeros(G.shape[0], dtype=torch.bool, device=G.device)
    for z in pre:
        near |= (z.abs() < 1e-5 * z.abs().max()).any(dim=1).to(G.device)
    frac = float(near.float().mean())
    print(f'[fusedmlp] {tag}: {int(near.sum())} of {G.shape[0]} rows near a kink dropped from the gradients ({100 * frac:.2f} %)')
    assert frac <= 0.10, (tag, frac)
    G = G.clone()
    G[near] = 0.0
    return G, frac


def run_ref(dev, x, ws, cfg, G, mask=None, scale=None, bias=None, in_grad_scale=1.0):
    """value, d_x, [d_w] of the restatement on `dev`, and the upstream gradient with its near-kink rows zeroed"""
    mv = lambda t: None if t is None else t.to(dev)
    xr = x.clone().to(dev).requires_grad_(True)
    wr = [w.clone().to(dev).double().requires_grad_(True) for w in ws]
    pre = []
    o = ref_mlp(xr, wr, cfg, mv(mask), mv(scale), mv(bias), in_grad_scale, pre)
    G, _ = drop_kinks(G.to(dev), pre, repr(cfg))
    if x.shape[0]:
        (o * G.double()).sum().backward()
    dx = xr.grad if xr.grad is not None else torch.zeros_like(xr)
    return (o.detach(), dx, [w.grad if w.grad is not None else torch.zeros_like(w) for w in wr]), G


def run_kernel(dev, x, ws, cfg, G, mask=None, scale=None, bias=None, in_grad_scale=1.0, max_cus=0, grad_x=True, grad_w=True):
    from d3h import fusedmlp
    mv = lambda t: None if t is None else t.to(dev)
    xa = x.clone().to(dev).requires_grad_(grad_x)
    wa = [w.clone().to(dev).requires_grad_(grad_w) for w in ws]
    o = fusedmlp.fused_mlp(xa, wa, cfg, mask=mv(mask), out_scale=mv(scale), out_bias=mv(bias), in_grad_scale=in_grad_scale, max_cus=max_cus)
    assert o.shape == (x.shape[0], cfg.n_output_dims) and o.dtype == torch.float32
    if grad_x or grad_w:
        (o * G.to(dev)).sum().backward()
    return o.detach(), xa.grad, [w.grad for w in wa]


def rel(a, b):
    if b.numel() == 0:
        return 0.0
    return float((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-30))


def compare(tag, got, ref):
    o, dx, dw = got
    orf, dxr, dwr = ref
    fig = {'out': rel(o, orf)}
    if dx is not None:
        fig['x'] = rel(dx, dxr)
    for l, (a, b) in enumerate(zip(dw, dwr)):
        if a is not None:
            fig[f'w{l}'] = rel(a, b)
    print(f'[fusedmlp] {tag}: {fig}')
    assert all(v < TOL_TEX for v in fig.values()), (tag, fig)
    return fig


def check_case(dev, shape, n, act='ReLU', out_act='None', seed=0, mask_frac=0.0, affine=False, in_grad_scale=1.0, max_cus=0, tag=None):
    from d3h import fusedmlp
    cfg = fusedmlp.MLPConfig(*net_cfg(shape, act, out_act))
    x, ws, G, mask, scale, bias = make_state(cfg, n, seed, mask_frac, affine)
    ref, G = run_ref(dev, x, ws, cfg, G, mask, scale, bias, in_grad_scale)
    got = run_kernel(dev, x, ws, cfg, G, mask, scale, bias, in_grad_scale, max_cus)
    compare(tag or f'{shape} {act}/{out_act} n={n}', got, ref)
    return cfg, (x, ws, G, mask, scale, bias), got, ref


# ---- 1. the shape matrix -----------------------------------------------------------------------------------------------------------------------
def check_shape(dev, shape):
    """N = 257 and N = 1000: ragged against any tile size, more than one workgroup"""
    for n in (257, 1000):
        check_case(dev, shape, n, seed=sum(shape) + n)


# ---- 2. row counts -----------------------------------------------------------------------------------------------------------------------------
def check_row_counts(dev, n_walk):
    from d3h import fusedmlp
    shape = (32, 64, 3, 9)
    for n in (0, 1, 63, 64, 65):
        _, _, got, _ = check_case(dev, shape, n, seed=200 + n)
        if n == 0:
            assert got[0].shape == (0, 9) and got[1].shape == (0, 32) and all(float(w.abs().max()) == 0.0 for w in got[2])
    # one workgroup walks every tile: its partial d_w survives the loop
    cfg, (x, ws, G, *_), one, ref = check_case(dev, shape, n_walk, seed=77, max_cus=1, tag=f'{shape} n={n_walk} max_cus=1')
    allc = run_kernel(dev, x, ws, cfg, G, max_cus=0)
    compare(f'{shape} n={n_walk} max_cus=1 vs max_cus=0', one, allc)


# ---- 3. activations ----------------------------------------------------------------------------------------------------------------------------
def check_hidden_activations(dev, n=300):
    for k, act in enumerate(ACT):
        check_case(dev, (7, 32, 2, 3), n, act=act, seed=300 + k)


def check_output_activations(dev, n=400):
    from d3h import fusedmlp
    for k, out_act in enumerate(ACT):
        cfg, (x, ws, G, mask, scale, bias), got, _ = check_case(dev, (32, 32, 2, 6), n, out_act=out_act, seed=400 + k, mask_frac=0.2, affine=True,
                                                                in_grad_scale=128.0)
        dead = (mask <= 0).to(dev)
        assert 0.1 < float(dead.float().mean()) < 0.3
        assert float(got[0][dead].abs().max()) == 0.0 and float(got[1][dead].abs().max()) == 0.0       # exactly zero rows
        assert float(got[1][~dead].abs().max()) > 0.0
        keep = mask > 0
        comp = run_kernel(dev, x[keep], ws, cfg, G.cpu()[keep], None, scale, bias, 128.0)
        fig = {f'w{l}': rel(a, b) for l, (a, b) in enumerate(zip(got[2], comp[2]))}
        print(f'[fusedmlp] output {out_act}: d_w against the compacted rows {fig}')
        assert all(v < TOL_TEX for v in fig.values()), fig
        assert torch.equal(got[0][~dead], comp[0])


# ---- 4. accumulation (the C ABI itself) ----------------------------------------------------------------------------------------------------------
def _raw_bwd(dev, cfg, x, ws, G, d_x, d_w):
    from d3h import _lib as L
    arr = lambda ts: (ctypes.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])
    rc = L.lib().d3h_fusedmlp_bwd(L.ptr(x), L.i64(x.shape[0]), *cfg._kernel_args(), arr(ws), None, None, L.ptr(G), L.f32(1.0), L.ptr(d_x),
                                  arr(d_w), L.i32(0), L.stream())
    L.check(rc, 'fusedmlp_bwd')


def check_accumulation(dev, n=500):
    from d3h import fusedmlp
    shape = (32, 64, 3, 9)
    cfg = fusedmlp.MLPConfig(*net_cfg(shape))
    x, ws, G, *_ = make_state(cfg, n, 500)
    x, G, ws = x.to(dev), G.to(dev), [w.to(dev) for w in ws]
    once = [torch.zeros_like(w) for w in ws]
    dx1 = torch.empty_like(x)
    _raw_bwd(dev, cfg, x, ws, G, dx1, once)
    twice = [torch.zeros_like(w) for w in ws]
    dx2 = torch.full_like(x, 777.0)                          # d_x is overwritten: the fill leaves no trace
    _raw_bwd(dev, cfg, x, ws, G, dx2, twice)
    _raw_bwd(dev, cfg, x, ws, G, dx2, twice)
    fig = {f'w{l}': rel(b, 2.0 * a) for l, (a, b) in enumerate(zip(once, twice))}
    print(f'[fusedmlp] two backward calls into the same d_w against twice one call: {fig}')
    assert all(v < TOL_TEX for v in fig.values()) and all(float(a.abs().max()) > 0 for a in once), fig
    assert torch.equal(dx1, dx2)
    # entries of the pointer array may be NULL, and so may the array
    some = [torch.zeros_like(w) if l % 2 == 0 else None for l, w in enumerate(ws)]
    _raw_bwd(dev, cfg, x, ws, G, None, some)
    for l, (a, b) in enumerate(zip(once, some)):
        assert b is None or rel(b, a) < TOL_TEX, l
    from d3h import _lib as L
    dx3 = torch.full_like(x, -3.0)
    L.check(L.lib().d3h_fusedmlp_bwd(L.ptr(x), L.i64(n), *cfg._kernel_args(), (ctypes.c_void_p * 4)(*[w.data_ptr() for w in ws]), None, None,
                                     L.ptr(G), L.f32(1.0), L.ptr(dx3), None, L.i32(0), L.stream()), 'fusedmlp_bwd')
    assert torch.equal(dx1, dx3)


# ---- 5. validation before any launch -------------------------------------------------------------------------------------------------------------
def check_validation(dev, monkeypatch):
    from d3h import fusedmlp, _lib as L
    import tinycudann as tcnn
    lib = L.lib()
    launches = {'n': 0}
    for name in ('d3h_fusedmlp_fwd', 'd3h_fusedmlp_bwd'):
        real = getattr(lib, name)
        monkeypatch.setattr(lib, name, lambda *a, _r=real: (launches.__setitem__('n', launches['n'] + 1), _r(*a))[1], raising=False)
    base = {'otype': 'FullyFusedMLP', 'n_neurons': 32, 'n_hidden_layers': 2}
    for mk in (fusedmlp.MLPConfig, tcnn.Network):
        for n_in, n_out, c, err, key in ((8, 3, dict(base, otype='ResNet'), NotImplementedError, 'otype'),
                                         (8, 3, dict(base, activation='Sine'), NotImplementedError, 'activation'),
                                         (8, 3, dict(base, activation='Squareplus'), NotImplementedError, 'activation'),
                                         (8, 3, dict(base, output_activation='Sine'), NotImplementedError, 'output_activation'),
                                         (8, 3, dict(base, n_neurons=48), NotImplementedError, 'n_neurons'),
                                         (8, 3, dict(base, n_neurons=256), NotImplementedError, 'n_neurons'),
                                         (8, 3, dict(base, n_hidden_layers=0), ValueError, 'n_hidden_layers'),
                                         (8, 3, dict(base, n_hidden_layers=-1), ValueError, 'n_hidden_layers'),
                                         (8, 3, dict(base, n_hidden_layers=9), ValueError, 'n_hidden_layers'),
                                         (0, 3, base, ValueError, 'n_input_dims'), (257, 3, base, ValueError, 'n_input_dims'),
                                         (8, 0, base, ValueError, 'n_output_dims'), (8, 129, base, ValueError, 'n_output_dims')):
            with pytest.raises(err, match=key):
                mk(n_in, n_out, c)
    # tcnn's defaults
    d = fusedmlp.MLPConfig(3, 4, {})
    assert (d.n_neurons, d.n_hidden_layers, d.activation, d.output_activation) == (128, 5, 'ReLU', 'None') and len(d.shapes) == 6
    assert fusedmlp.MLPConfig(3, 4, {'otype': 'CutlassMLP'}).n_params == d.n_params == 128 * 3 + 4 * 128 * 128 + 4 * 128
    cfg = fusedmlp.MLPConfig(8, 3, base)
    x, ws, G, *_ = make_state(cfg, 5, 1)
    x, ws = x.to(dev), [w.to(dev) for w in ws]
    with pytest.raises(ValueError, match='columns'):
        fusedmlp.fused_mlp(torch.rand(5, 7).to(dev), ws, cfg)
    with pytest.raises(ValueError, match='shape'):
        fusedmlp.fused_mlp(x, [ws[0], ws[1].t().contiguous()[:, :31].contiguous(), ws[2]], cfg)
    with pytest.raises(ValueError, match='weight matrices'):
        fusedmlp.fused_mlp(x, ws[:2], cfg)
    with pytest.raises(ValueError, match='mask'):
        fusedmlp.fused_mlp(x, ws, cfg, mask=torch.ones(4).to(dev))
    with pytest.raises(ValueError, match='out_scale'):
        fusedmlp.fused_mlp(x, ws, cfg, out_scale=torch.ones(4).to(dev))
    assert launches['n'] == 0
    # the C ABI refuses what the host module would: no launch behind any of these either (the return code comes first)
    out = torch.empty(5, 3).to(dev)
    warr = (ctypes.c_void_p * 3)(*[w.data_ptr() for w in ws])
    call = lambda x_=x, n=5, n_in=8, width=32, hidden=2, n_out=3, act=1, oact=0, w=warr, out_=out: real_fwd(
        None if x_ is None else ctypes.c_void_p(x_ if isinstance(x_, int) else x_.data_ptr()), L.i64(n), L.i32(n_in), L.i32(width), L.i32(hidden),
        L.i32(n_out), L.i32(act), L.i32(oact), w, None, None, None, ctypes.c_void_p(out_.data_ptr()), L.i32(0), L.stream())
    real_fwd = lib.d3h_fusedmlp_fwd
    assert call() == 0
    assert call(n=0) == 0 and call(n=0, x_=None) == 0
    for kw in (dict(width=48), dict(width=256), dict(hidden=0), dict(hidden=9), dict(n_in=0), dict(n_in=257), dict(n_out=0), dict(n_out=129),
               dict(act=7), dict(oact=-1), dict(x_=None), dict(x_=x.data_ptr() + 2), dict(w=None), dict(n=-1),
               dict(w=(ctypes.c_void_p * 3)(ws[0].data_ptr(), None, ws[2].data_ptr()))):
        assert call(**kw) == -1, kw
    # first order only
    xa = x.clone().requires_grad_(True)
    o = fusedmlp.fused_mlp(xa, ws, cfg)
    with pytest.raises(RuntimeError, match='once_differentiable|differentiated twice|double backward'):
        (gx,) = torch.autograd.grad((o * o).sum(), xa, create_graph=True)
        gx.sum().backward()


# ---- 6. the shim ---------------------------------------------------------------------------------------------------------------------------------
def check_shim(dev):
    import tinycudann as tcnn
    from d3h import fusedmlp, gridenc, texmlp
    nc = {'otype': 'FullyFusedMLP', 'activation': 'ReLU', 'output_activation': 'None', 'n_neurons': 32, 'n_hidden_layers': 2}
    torch.manual_seed(5)                          # the parameters come from `seed`, not from the global generator
    a = tcnn.Network(20, 6, nc).to(dev)
    b = tcnn.Network(20, 6, nc, seed=1337).to(dev)
    other = tcnn.Network(20, 6, nc, seed=7).to(dev)
    assert a.n_input_dims == 20 and a.n_output_dims == 6
    assert isinstance(a.params, torch.nn.Parameter) and a.params.dtype == torch.float32 and a.params.shape == (32 * 20 + 32 * 32 + 6 * 32,)
    assert torch.equal(a.params, b.params) and not torch.equal(a.params, other.params)
    off = 0
    for fo, fi in ((32, 20), (32, 32), (6, 32)):
        m, bound = a.params.detach()[off:off + fo * fi], (6.0 / (fi + fo)) ** 0.5
        assert 0.9 * bound < float(m.abs().max()) <= bound and float(m.min()) < 0 < float(m.max()), (fo, fi)
        off += fo * fi
    x = (torch.rand(70, 20) * 2 - 1).to(dev)
    y = a(x)
    assert y.shape == (70, 6) and y.dtype == torch.float32
    assert torch.equal(y, fusedmlp.fused_mlp(x, [a.params[:640].view(32, 20), a.params[640:1664].view(32, 32), a.params[1664:].view(6, 32)], a.cfg))
    ref = ref_mlp(x, [a.params.detach()[:640].view(32, 20), a.params.detach()[640:1664].view(32, 32), a.params.detach()[1664:].view(6, 32)], a.cfg)
    assert rel(y.detach(), ref) < TOL_TEX
    y.sum().backward()
    assert a.params.grad is not None and a.params.grad.shape == a.params.shape and float(a.params.grad.abs().max()) > 0
    d = tcnn.Network(3, 4, {'otype': 'CutlassMLP'})
    assert d.params.numel() == 128 * 3 + 4 * 128 * 128 + 4 * 128
    # with an input encoding: one flat vector, the network first, then the table
    ec = {'otype': 'HashGrid', 'n_levels': 6, 'n_features_per_level': 4, 'log2_hashmap_size': 10, 'base_resolution': 8, 'per_level_scale': 1.6}
    for enc_cfg, n_enc in ((ec, 24), (REF_CFG, 10)):
        nw = tcnn.NetworkWithInputEncoding(3, 5, enc_cfg, nc).to(dev)
        net, enc = tcnn.Network(n_enc, 5, nc).to(dev), tcnn.Encoding(3, enc_cfg).to(dev)
        assert nw.n_input_dims == 3 and nw.n_output_dims == 5 and nw.params.dtype == torch.float32
        assert torch.equal(nw.params, torch.cat([net.params, enc.params]))
        assert (nw.enc_cfg is None) == (enc_cfg is REF_CFG)
        n_net = net.params.numel()
        xs = torch.rand(90, 3).to(dev)
        with torch.no_grad():
            nw.params[n_net:] = (torch.rand(enc.params.numel()) - 0.5).to(dev)       # (features of 1e-4 would leave the output near zero)
        y = nw(xs)
        assert y.shape == (90, 5) and y.dtype == torch.float32
        table = nw.params[n_net:]
        e = texmlp.grid_encode(xs, table) if enc_cfg is REF_CFG else gridenc.grid_encode(xs, table, nw.enc_cfg)
        mats, o = [], 0
        for fo, fi in net.cfg.shapes:
            mats.append(nw.params[o:o + fo * fi].view(fo, fi))
            o += fo * fi
        assert torch.equal(y, fusedmlp.fused_mlp(e, mats, nw.cfg))
        (y * torch.randn(90, 5).to(dev)).sum().backward()
        gr = nw.params.grad
        assert gr.shape == nw.params.shape and float(gr[:n_net].abs().max()) > 0 and float(gr[n_net:].abs().max()) > 0


# ---- 7. the texture --------------------------------------------------------------------------------------------------------------------------------
def _texture_pair(dev, monkeypatch, n, enc_cfg, shape, calls):
    """the same general state on the fused network and (D3H_TEX_FUSED_NET=0) on the library GEMMs: value and every gradient"""
    from render.mlptexture import MLPTexture3D
    gen = torch.Generator().manual_seed(61)
    C = shape.get('channels', 6)
    lo, hi = torch.rand(C, generator=gen) * 0.1, 0.5 + torch.rand(C, generator=gen)
    mk = lambda: MLPTexture3D(None, min_max=[lo.to(dev), hi.to(dev)], enc_cfg=enc_cfg, **dict({'channels': 6}, **shape)).to(dev)
    monkeypatch.setenv('D3H_TEX_FUSED_NET', '1')
    tex = mk()
    assert tex.fused_net and not tex.fused
    monkeypatch.setenv('D3H_TEX_FUSED_NET', '0')
    lib_tex = mk()
    monkeypatch.delenv('D3H_TEX_FUSED_NET', raising=False)
    # not set: the library path, until the probe's measurement on the MI355X earns the fused network the default (render/mlptexture.py)
    assert not mk().fused_net
    assert not lib_tex.fused_net and not lib_tex.fused and sorted(lib_tex.state_dict()) == sorted(tex.state_dict())
    with torch.no_grad():
        tex.encoder.params.copy_((torch.rand(tex.encoder.params.numel(), generator=gen) - 0.5).to(dev))
    lib_tex.load_state_dict(tex.state_dict())
    texc = (torch.rand(n, 3, generator=gen) * torch.tensor([1.8, 2.2, 0.6]) + torch.tensor([-1.0, -1.4, -0.3])).to(dev)     # partly outside the box
    mask = (torch.rand(n, generator=gen) > 0.2).float().to(dev)
    G = torch.randn(n, C, generator=gen).to(dev)
    # near-kink rows of the upstream gradient, from a float64 evaluation of the network on the encoding
    with torch.no_grad():
        b0, b1 = torch.tensor(tex.BBOX[:3], device=dev), torch.tensor(tex.BBOX[3:], device=dev)
        h = tex.encoder(torch.clamp((texc - b0[None]) / (b1 - b0)[None], min=0, max=1).contiguous()).double()
        pre = []
        for m in [m for m in tex.net.net if isinstance(m, torch.nn.Linear)][:-1]:
            pre.append(h @ m.weight.double().t())
            h = torch.relu(pre[-1])
    G, _ = drop_kinks(G, pre, f'texture {shape}')
    res = []
    for t in (tex, lib_tex):
        before = calls['n']
        xa = texc.clone().requires_grad_(True)
        out = t.sample(xa.reshape(n // 4, 4, 3), None, mask=mask.reshape(n // 4, 4))
        assert out.shape == (n // 4, 4, C) and out.dtype == torch.float32
        assert calls['n'] - before == (1 if t is tex else 0)                   # one fused_mlp call per sample(); none on the library path
        (out.reshape(n, C) * G).sum().backward()
        res.append((out.detach().reshape(n, C), xa.grad, t.encoder.params.grad, [m.weight.grad for m in t.net.net if isinstance(m, torch.nn.Linear)]))
    (o, dx, dt, dw), (o2, dx2, dt2, dw2) = res
    assert float(o[mask <= 0].abs().max()) == 0.0 and float(dx[mask <= 0].abs().max()) == 0.0
    fig = {'out': rel(o, o2), 'texc': rel(dx, dx2), 'table': rel(dt, dt2)}
    for l, (a, b) in enumerate(zip(dw, dw2)):
        fig[f'w{l}'] = rel(a, b)
    print(f'[fusedmlp] texture {enc_cfg} {shape}: fused network against the library GEMMs {fig}')
    assert all(v < TOL_TEX for v in fig.values()), fig
    assert float(dx2.abs().max()) > 0 and float(dt2.abs().max()) > 0


def check_texture(dev, monkeypatch, n, T=14):
    from d3h import fusedmlp
    from render.mlptexture import MLPTexture3D
    calls = {'n': 0}
    real = fusedmlp.fused_mlp
    monkeypatch.setattr(fusedmlp, 'fused_mlp', lambda *a, **k: (calls.__setitem__('n', calls['n'] + 1), real(*a, **k))[1])
    _texture_pair(dev, monkeypatch, n, cfg16(T), {}, calls)
    _texture_pair(dev, monkeypatch, n, None, dict(channels=9, internal_dims=64, hidden=3), calls)
    # a width the kernels are not built for stays on the library path, silently
    mm = [torch.zeros(6).to(dev), torch.ones(6).to(dev)]
    monkeypatch.setenv('D3H_TEX_FUSED_NET', '1')
    odd = MLPTexture3D(None, channels=6, internal_dims=48, min_max=mm).to(dev)
    before = calls['n']
    assert not odd.fused_net and not odd.fused
    assert odd.sample(torch.rand(4, 5, 3).to(dev) - 0.5).shape == (4, 5, 6) and calls['n'] == before
    # and the reference's shape stays on csrc/texmlp.hip
    ref = MLPTexture3D(None, channels=6, min_max=mm).to(dev)
    assert ref.fused and not ref.fused_net
    assert ref.sample(torch.rand(4, 5, 3).to(dev) - 0.5).shape == (4, 5, 6) and calls['n'] == before
