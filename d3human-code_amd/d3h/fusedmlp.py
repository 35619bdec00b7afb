"""Host side of csrc/fusedmlp.hip: the general fused bias-free MLP behind `tinycudann.Network` / `NetworkWithInputEncoding` and the
general texture network of render/mlptexture.py.

PARITY UNPINNED: tiny-cuda-nn is not vendored by the reference (README.md:30), so -- as d3h/gridenc.py does for the encoding -- this
restates the library's published network (FullyFusedMLP / CutlassMLP: no biases, one activation for the hidden layers, one for the output)
from memory; parity with the real library is not pinned.  What IS pinned: the float64 restatement of tests/fusedmlp_cases.py and, through
MLPTexture3D, the float64 restatement of the reference's sample() in tests/gridenc_cases.py:check_texture.  Known deviations: float32
parameters and output (tcnn: half precision); the parameters are the matrices with their exact shapes (tcnn pads the first fan-in and the
last fan-out to 16 inside its vector); `Softplus` is log(1 + e^z) (recalled: tcnn sharpens it by a constant factor).

The contract.  `n_input_dims` 1..256 -> `n_hidden_layers` (1..8) hidden layers of `n_neurons` (16 | 32 | 64 | 128) -> `n_output_dims`
1..128: `n_hidden_layers + 1` matrices M_l in nn.Linear layout [fan_out][fan_in], float32, and

  * `h <- activation(h @ M_l.T)` for every matrix but the last, `z = h @ M_L.T`, `out = output_activation(z) * out_scale + out_bias`
    (`out_scale`, `out_bias`: None or [n_output_dims] constants without a gradient -- the sigmoid range map of render/mlptexture.py);
  * activations: "None", "ReLU", "LeakyReLU" (slope 0.01), "Sigmoid", "Tanh", "Softplus", "Exponential";
  * `mask` None or [N]: a row with `mask <= 0` gives a zero output row, a zero row of d_x and adds nothing to any d_w;
  * every dot product is an fmaf chain in float32 (the exact-f32 matrix instruction), summed in a fixed order per row;
  * gradients, FIRST ORDER ONLY (`once_differentiable`: a double backward raises): the backward keeps NO activation -- it reads x, the
    matrices and the incoming gradient and recomputes the forward of each tile (the derivative of every activation above is a function of
    its value).  d_x is multiplied by `in_grad_scale` (the x128 hook of the reference's _MLP).  The matrices' gradients are summed per
    workgroup and flushed once with float atomics: their last bits depend on the order of arrival.
  * N = 0 returns empty tensors without a launch.

`network_config` keys (tcnn's names and defaults): `otype` "FullyFusedMLP" | "CutlassMLP" (the same kernels), `activation` "ReLU",
`output_activation` "None", `n_neurons` 128, `n_hidden_layers` 5.  NotImplementedError (naming the key): other otypes, other activations
("Sine", "Squareplus"), other widths.  ValueError: a non-positive or out-of-range `n_hidden_layers`, `n_input_dims`, `n_output_dims`.
"""

import torch
from torch.autograd.function import once_differentiable

from . import _lib as L

ACTIVATIONS = {'None': 0, 'ReLU': 1, 'LeakyReLU': 2, 'Sigmoid': 3, 'Tanh': 4, 'Softplus': 5, 'Exponential': 6}
WIDTHS = (16, 32, 64, 128)
MAX_HIDDEN, MAX_IN, MAX_OUT = 8, 256, 128


def _activation(key, name):
    name = 'None' if name is None else name
    if name not in ACTIVATIONS:
        raise NotImplementedError(f'd3h fused MLP: {key} {name!r} is not built ({", ".join(ACTIVATIONS)})')
    return name


def _count(key, v, hi):
    if isinstance(v, bool) or int(v) != v or v < 1 or v > hi:
        raise ValueError(f'd3h fused MLP: {key} must be an integer in 1..{hi} (got {v})')
    return int(v)


def supported(n_input_dims, n_output_dims, n_neurons, n_hidden_layers):
    """whether the kernels are built for this shape (render/mlptexture.py routes by it)"""
    return (n_neurons in WIDTHS and 1 <= n_hidden_layers <= MAX_HIDDEN and 1 <= n_input_dims <= MAX_IN and 1 <= n_output_dims <= MAX_OUT)


class MLPConfig:
    """a parsed, validated `network_config`: n_input_dims, n_output_dims, n_neurons, n_hidden_layers, activation, output_activation, and
    `shapes`, the [fan_out, fan_in] of the n_hidden_layers + 1 matrices"""

    def __init__(self, n_input_dims, n_output_dims, network_config):
        c = dict(network_config)
        otype = c.get('otype', 'FullyFusedMLP')
        if otype not in ('FullyFusedMLP', 'CutlassMLP'):
            raise NotImplementedError(f'd3h fused MLP: otype {otype!r} is not built (FullyFusedMLP or CutlassMLP)')
        self.activation = _activation('activation', c.get('activation', 'ReLU'))
        self.output_activation = _activation('output_activation', c.get('output_activation', 'None'))
        nn_ = c.get('n_neurons', 128)
        if nn_ not in WIDTHS:
            raise NotImplementedError(f'd3h fused MLP: n_neurons {nn_} is not built (16, 32, 64 or 128)')
        self.n_neurons = int(nn_)
        self.n_hidden_layers = _count('n_hidden_layers', c.get('n_hidden_layers', 5), MAX_HIDDEN)
        self.n_input_dims = _count('n_input_dims', n_input_dims, MAX_IN)
        self.n_output_dims = _count('n_output_dims', n_output_dims, MAX_OUT)
        w, n = self.n_neurons, self.n_hidden_layers
        self.shapes = [(w, self.n_input_dims)] + [(w, w)] * (n - 1) + [(self.n_output_dims, w)]
        self.n_params = sum(a * b for a, b in self.shapes)

    def _kernel_args(self):
        return (self.n_input_dims, self.n_neurons, self.n_hidden_layers, self.n_output_dims, ACTIVATIONS[self.activation],
                ACTIVATIONS[self.output_activation])

    def __repr__(self):
        return (f'MLPConfig({self.n_input_dims} -> {self.n_neurons} x {self.n_hidden_layers} -> {self.n_output_dims}, {self.activation}, '
                f'output {self.output_activation}: {self.n_params} parameters)')


def _vec(v, n, dev, what):
    if v is None:
        return None
    v = torch.as_tensor(v, dtype=torch.float32, device=dev).detach().reshape(-1).contiguous()
    if v.numel() != n:
        raise ValueError(f'd3h fused MLP: {what} has {v.numel()} elements, the network {n} outputs')
    return v


class _FusedMLPFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, cfg, mask, out_scale, out_bias, in_grad_scale, max_cus, *weights):
        if x.shape[-1] != cfg.n_input_dims:
            raise ValueError(f'd3h fused MLP: x has {x.shape[-1]} columns, the network {cfg.n_input_dims} input dimensions')
        if len(weights) != len(cfg.shapes):
            raise ValueError(f'd3h fused MLP: {len(weights)} weight matrices, the network has {len(cfg.shapes)}')
        for l, (w, shp) in enumerate(zip(weights, cfg.shapes)):
            if tuple(w.shape) != shp:
                raise ValueError(f'd3h fused MLP: weight {l} has shape {tuple(w.shape)}, the network {shp}')
        xs = x.reshape(-1, cfg.n_input_dims).contiguous().float()
        ws = [w.detach().contiguous().float() for w in weights]
        n, dev = xs.shape[0], x.device
        mk = None
        if mask is not None:
            mk = mask.detach().reshape(-1).contiguous().float()
            if mk.numel() != n:
                raise ValueError(f'd3h fused MLP: mask has {mk.numel()} elements, x {n} rows')
        sc, bi = _vec(out_scale, cfg.n_output_dims, dev, 'out_scale'), _vec(out_bias, cfg.n_output_dims, dev, 'out_bias')
        out = torch.empty(n, cfg.n_output_dims, dtype=torch.float32, device=dev)
        if n > 0:
            L.call('fusedmlp_fwd', xs, n, *cfg._kernel_args(), L.ptr_array(ws), mk, sc, bi, out, max_cus)
        ctx.save_for_backward(xs, *ws)                     # inputs only: no activation is kept
        ctx.cfg, ctx.mask, ctx.scale, ctx.xshape, ctx.in_grad_scale, ctx.max_cus = cfg, mk, sc, x.shape, float(in_grad_scale), int(max_cus)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        xs, *ws = ctx.saved_tensors
        cfg, n = ctx.cfg, xs.shape[0]
        need_w = list(ctx.needs_input_grad[7:])
        d_x = torch.empty_like(xs) if ctx.needs_input_grad[0] else None
        d_w = [L.zeros_like(w) if nw else None for w, nw in zip(ws, need_w)]
        if n > 0 and (d_x is not None or any(need_w)):
            gc = g.reshape(n, cfg.n_output_dims).contiguous().float()
            L.call('fusedmlp_bwd', xs, n, *cfg._kernel_args(), L.ptr_array(ws), ctx.mask, ctx.scale, gc, ctx.in_grad_scale, d_x,
                   L.ptr_array(d_w) if any(need_w) else None, ctx.max_cus)
        return (d_x.reshape(ctx.xshape) if d_x is not None else None, None, None, None, None, None, None) + tuple(d_w)


def fused_mlp(x, weights, cfg, mask=None, out_scale=None, out_bias=None, in_grad_scale=1.0, max_cus=0):
    """x [..., n_input_dims], weights: the cfg.n_hidden_layers + 1 matrices [fan_out, fan_in] -> [N, n_output_dims] float32 on the current
    stream (see the module docstring).  `max_cus` > 0 caps the persistent grid at that many workgroups (tests; 0: the whole chip)."""
    return _FusedMLPFn.apply(x, cfg, mask, out_scale, out_bias, in_grad_scale, max_cus, *weights)
