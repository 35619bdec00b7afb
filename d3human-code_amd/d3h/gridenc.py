"""Host side of csrc/gridenc.hip: the general multiresolution grid encoding behind `tinycudann.Encoding` (HashGrid / DenseGrid).

PARITY UNPINNED: tiny-cuda-nn is not vendored by the reference (README.md:30), so -- as csrc/texmlp.hip and oracle/texmlp.py do for the one
dense configuration of render/mlptexture.py:62-75 -- this restates the library's published algorithm from memory; parity with the real
library is not pinned.  What IS pinned: tests/gridenc_cases.py:ref_encode (a float64 restatement of the contract below) and, on the
reference configuration, oracle/texmlp.py and the fused kernels of csrc/texmlp.hip.

The contract.  Input dimension D in {2, 3}, levels L in 1..32, features per entry F in {1, 2, 4, 8}, `log2_hashmap_size` T,
`base_resolution` B, `per_level_scale` s:

  * level l: `scale = exp2f(l * log2f(s)) * B - 1` in float32, `res = ceil(scale) + 1`, entries `n_l = round_up(res^D, 8)`, for grid type Hash
    then `min(n_l, 2^T)`.  Level offsets are the running sum; the parameter vector is `sum(n_l) * F` float32, entry-major inside a level (the F
    features of an entry are contiguous).  The layout is computed in ONE place, `d3h_gridenc_layout` of the library, which the kernels'
    entry points use as well.
  * position: `p = fmaf(x, scale, 0.5)` in float32, cell `floor(p)`, fraction `fr = p - floor(p)`; the 2^D corners of the cell, corner bit d
    taken from bit d of the corner number.
  * entry of an integer corner q (uint32 arithmetic): `idx = sum_d q_d * res^d`; when `res^D > n_l` (only possible for type Hash) the level is
    HASHED and `idx = q_0 * 1 ^ q_1 * 2654435761 ^ q_2 * 805459861`; in both cases the entry is `idx % n_l`.  For a dense level this is the
    wrap the fused kernel does (x == 1 on level 0 reaches corner `res`).
  * weight of a corner: product over d of `w_d` or `1 - w_d`; interpolation "Linear": `w = fr`; "Smoothstep": `w = fr^2 (3 - 2 fr)`,
    `dw/dfr = 6 fr (1 - fr)`.  Output `[N, L * F]` float32, column `l * F + f` (tcnn's default half-precision output is a documented
    deviation of the shim already).
  * gradients, FIRST ORDER ONLY (`once_differentiable`: a double backward raises): to the table, sum over points and corners of `w * g`; to x,
    `scale * sum_corners (+-) prod_{e != d} w_e * dw_d/dfr * <feat, g>`.  Both are sums of float atomics: the last bits depend on the order
    of arrival.
  * inputs are expected in [0, 1]^D and are NOT clamped (tcnn does not clamp).  Every index is reduced `% n_l` as an unsigned number, so any
    float32 input, non-finite included, reads and adds inside the table: a point outside the unit cube gives an unspecified row, never an
    out-of-bounds access (argued in the header comment of csrc/gridenc.hip).  N = 0 returns empty tensors without a launch.

`encoding_config` keys (tcnn's names and defaults): `otype` "HashGrid" | "DenseGrid" | "Grid", `type` "Hash" | "Dense" (default from the
otype), `n_levels` 16, `n_features_per_level` 2, `log2_hashmap_size` 19, `base_resolution` 16, `per_level_scale` 2.0, `interpolation`
"Linear" | "Smoothstep".  NotImplementedError (naming the key): D outside {2, 3}, F outside {1, 2, 4, 8}, `type` "Tiled", `interpolation`
"Nearest", other otypes.  ValueError: non-positive level count / resolution / scale, more than 32 levels, a table of 2^31 entries or more.
"""
import ctypes

import torch
from torch.autograd.function import once_differentiable

from . import _lib as L

_OTYPE_DEFAULT = {'HashGrid': 'Hash', 'DenseGrid': 'Dense', 'Grid': 'Hash', 'TiledGrid': 'Tiled'}
MAX_LEVELS = 32


class GridConfig:
    """a parsed, validated `encoding_config` with its table layout (per level: scale, res, offset, size, hashed; n_entries, n_params)"""

    def __init__(self, n_input_dims, encoding_config):
        c = dict(encoding_config)
        otype = c.get('otype', 'HashGrid')
        if otype not in _OTYPE_DEFAULT:
            raise NotImplementedError(f"d3h grid encoding: otype {otype!r} is not built (HashGrid, DenseGrid or Grid)")
        gtype = c.get('type', _OTYPE_DEFAULT[otype])
        if gtype not in ('Hash', 'Dense'):
            raise NotImplementedError(f"d3h grid encoding: type {gtype!r} is not built (Hash or Dense)")
        interp = c.get('interpolation', 'Linear')
        if interp not in ('Linear', 'Smoothstep'):
            raise NotImplementedError(f"d3h grid encoding: interpolation {interp!r} is not built (Linear or Smoothstep)")
        if n_input_dims not in (2, 3):
            raise NotImplementedError(f'd3h grid encoding: n_input_dims {n_input_dims} is not built (2 or 3)')
        nf = c.get('n_features_per_level', 2)
        if nf not in (1, 2, 4, 8):
            raise NotImplementedError(f'd3h grid encoding: n_features_per_level {nf} is not built (1, 2, 4 or 8)')
        nl, t_, base, pls = c.get('n_levels', 16), c.get('log2_hashmap_size', 19), c.get('base_resolution', 16), float(c.get('per_level_scale', 2.0))
        if int(nl) != nl or nl < 1:
            raise ValueError(f'd3h grid encoding: n_levels must be a positive integer (got {nl})')
        if nl > MAX_LEVELS:
            raise ValueError(f'd3h grid encoding: n_levels {nl} exceeds the {MAX_LEVELS} levels of a launch')
        if int(base) != base or base < 1:
            raise ValueError(f'd3h grid encoding: base_resolution must be a positive integer (got {base})')
        if not pls > 0.0 or pls == float('inf'):
            raise ValueError(f'd3h grid encoding: per_level_scale must be positive and finite (got {pls})')
        if int(t_) != t_ or t_ < 0:
            raise ValueError(f'd3h grid encoding: log2_hashmap_size must be a non-negative integer (got {t_})')
        too_large = ValueError(f'd3h grid encoding: the table would have 2^31 entries or more (n_levels {nl}, base_resolution {base}, '
                               f'per_level_scale {pls}, log2_hashmap_size {t_}, type {gtype})')
        if t_ > 31:
            raise too_large
        self.n_dims, self.n_levels, self.n_features, self.log2_hashmap_size = int(n_input_dims), int(nl), int(nf), int(t_)
        self.base_resolution, self.per_level_scale, self.grid_type, self.interpolation = int(base), pls, gtype, interp
        self.n_output_dims = self.n_levels * self.n_features
        n = self.n_levels
        scale, res, hashed = (ctypes.c_float * n)(), (ctypes.c_int * n)(), (ctypes.c_int * n)()
        offset, size, total = (ctypes.c_int64 * n)(), (ctypes.c_int64 * n)(), ctypes.c_int64(0)
        try:
            L.call('gridenc_layout', *self._cfg_args(), scale, res, offset, size, hashed, ctypes.byref(total))
        except L.StatusError as e:
            if e.code == -2:
                raise too_large from None
            raise ValueError(f'd3h grid encoding: the library refuses this configuration (a level scale out of range?): {c}') from None
        self.scale, self.res, self.offset, self.size = [float(v) for v in scale], list(res), list(offset), list(size)
        self.hashed = [bool(v) for v in hashed]
        self.n_entries = int(total.value)
        self.n_params = self.n_entries * self.n_features

    def _cfg_args(self):
        return (self.n_dims, self.n_levels, self.n_features, self.log2_hashmap_size, self.base_resolution, self.per_level_scale,
                0 if self.grid_type == 'Hash' else 1)

    def _kernel_args(self):
        return self._cfg_args() + (0 if self.interpolation == 'Linear' else 1,)

    def __repr__(self):
        return (f'GridConfig(D={self.n_dims}, L={self.n_levels}, F={self.n_features}, T={self.log2_hashmap_size}, base={self.base_resolution}, '
                f'scale={self.per_level_scale}, {self.grid_type}, {self.interpolation}: {self.n_entries} entries, {sum(self.hashed)} hashed levels)')


def _aligned(t, nf):
    """the kernels fetch an entry as one vector: a view that starts inside an entry is copied"""
    return t if t.data_ptr() % (4 * nf) == 0 else t.clone()


class _GridEncFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, table, cfg):
        if x.shape[-1] != cfg.n_dims:
            raise ValueError(f'd3h grid encoding: x has {x.shape[-1]} columns, the encoding {cfg.n_dims} input dimensions')
        if table.numel() != cfg.n_params:
            raise ValueError(f'd3h grid encoding: the table has {table.numel()} floats, the configuration {cfg.n_params}')
        xs = x.reshape(-1, cfg.n_dims).contiguous().float()
        tab = _aligned(table.reshape(-1).contiguous().float(), cfg.n_features)
        n = xs.shape[0]
        out = torch.empty(n, cfg.n_output_dims, dtype=torch.float32, device=x.device)
        if n > 0:
            L.call('gridenc_fwd', xs, tab, tab.numel(), n, *cfg._kernel_args(), out)
        ctx.save_for_backward(xs, tab)
        ctx.cfg, ctx.xshape, ctx.tshape = cfg, x.shape, table.shape
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        xs, tab = ctx.saved_tensors
        cfg = ctx.cfg
        n = xs.shape[0]
        d_x = torch.zeros_like(xs) if ctx.needs_input_grad[0] else None
        d_tab = L.zeros_like(tab) if ctx.needs_input_grad[1] else None
        if n > 0 and (d_x is not None or d_tab is not None):
            gc = _aligned(g.reshape(n, cfg.n_output_dims).contiguous().float(), cfg.n_features)
            L.call('gridenc_bwd', xs, tab, tab.numel(), gc, n, *cfg._kernel_args(), d_tab, d_x)
        return (d_x.reshape(ctx.xshape) if d_x is not None else None, d_tab.reshape(ctx.tshape) if d_tab is not None else None, None)


def grid_encode(x, table, cfg):
    """x [..., D] (expected in [0, 1]) , table [cfg.n_params] float32 -> [N, L * F] float32 on the current stream (see the module docstring)"""
    return _GridEncFn.apply(x, table, cfg)
