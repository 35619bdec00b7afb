"""nvdiffrast.texture, the whole op: mip pyramids, four filter modes, four boundary modes, gradients for every input (csrc/texture.hip).

nvdiffrast is not vendored, so the op is pinned to this contract (restated in float64 torch by tests/test_texture_modes.py):

Shapes.  2-D: tex [B|1, H, W, C], uv [B, h, w, 2], uv_da [B, h, w, 4] = (du/dX, du/dY, dv/dX, dv/dY) (the `out_da` layout of
  d3h.raster.interpolate).  Cube: tex [B|1, 6, H, H, C], uv a direction [B, h, w, 3].  mip_level_bias [B, h, w].  Any C.  A texture batch
  of 1 is broadcast over the lookups.
Filter modes.  'nearest', 'linear', 'linear-mipmap-nearest', 'linear-mipmap-linear'; 'auto' is 'linear-mipmap-linear' when uv_da or
  mip_level_bias is given, 'linear' otherwise.  The mip modes need uv_da or mip_level_bias.
Texel centres at (i + 0.5) / N, u along W, v along H.  Nearest reads texel floor(u W); linear blends the 2 x 2 texels around u W - 0.5.
Boundary modes.  'wrap': positive modulo per tap; 'clamp': the index is clamped; 'zero': taps outside read 0 and receive no gradient;
  'cube': see below.
Pyramid.  Level l + 1 is the 2 x 2 box average of level l (a dimension of 1 stays 1 and the average runs over the other one).  Construction
  stops before a level whose parent has a dimension that is odd and greater than 1 (1080 x 1080 ends at 135 x 135), when both dimensions
  reach 1, at `max_mip_level` (the index of the last level), or at 16 levels.  `mip=` may instead give the levels below the base as a list
  (each [B|1, h, w, C] or [h, w, C]; cube [B|1, 6, h, h, C]) or a TextureMip from texture_construct_mip.
LOD.  level = 0.5 log2(lambda) + bias, lambda the larger eigenvalue of J^T J, J the 2 x 2 Jacobian of (u W0, v H0) w.r.t. (X, Y), clamped to
  [0, L - 1] (no gradient where clamped).  lambda = 0: level 0 with zero gradient.  -mipmap-nearest reads level floor(level + 0.5),
  -mipmap-linear blends floor(level) and floor(level) + 1 by the fraction.
Cube.  The face is the major axis of the direction (ties: x, then y, then z), faces ordered +x, -x, +y, -y, +z, -z; the face coordinates are
  the inverse of render/util.py:cube_to_dir.  A bilinear tap that leaves the face reads the texel of the adjacent face in the direction of
  that tap's centre; at a corner the missing fourth tap is the mean of the other three.  Nearest reads the face's own texel, clamped.  Cube
  maps take 'nearest', 'linear' and the mip modes driven by mip_level_bias; cube with uv_da raises NotImplementedError.
Gradients.  tex (into the base level, through the pyramid when it was built here; into each level when a list was given), uv (0 for
  'nearest'), uv_da and mip_level_bias (0 for '-mipmap-nearest'), each only when required.

The bilinear / clamp lookup without mips and without a uv gradient is d3h.raster.texture (nvdiffrast/torch.py routes it there)."""
import ctypes

import torch

from . import _lib as L

FILTERS = {'nearest': 0, 'linear': 1, 'linear-mipmap-nearest': 2, 'linear-mipmap-linear': 3}
BOUNDARIES = {'wrap': 0, 'clamp': 1, 'zero': 2, 'cube': 3}
MAX_LEVELS = 16                                  # csrc/texture.hip TEX_MAX_LEVELS


def mip_sizes(h, w, max_mip_level=None):
    """(H_l, W_l) of every level of the pyramid built from an h x w texture (see the module docstring)"""
    sizes = [(h, w)]
    while (h > 1 or w > 1) and (h == 1 or h % 2 == 0) and (w == 1 or w % 2 == 0) and len(sizes) < MAX_LEVELS:
        if max_mip_level is not None and len(sizes) > max_mip_level:
            break
        h, w = max(h // 2, 1), max(w // 2, 1)
        sizes.append((h, w))
    return sizes


def _hw(sizes):
    flat = [v for hw in sizes for v in hw]
    return (ctypes.c_int * len(flat))(*flat)


class TextureMip:
    """A built pyramid (texture_construct_mip): the packed level buffer (csrc/texture.hip) and its level sizes.  Gradients reach the
    texture it was built from when that texture required grad at construction time."""
    def __init__(self, pyr, sizes, bt, C, cube):
        self.pyr, self.sizes, self.bt, self.C, self.cube = pyr, sizes, bt, C, cube


class _MipBuildFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, tex, sizes, cube):
        tex = tex.contiguous().float()
        bt, C, F = tex.shape[0], tex.shape[-1], 6 if cube else 1
        pyr = torch.empty(sum(bt * F * h * w * C for h, w in sizes), dtype=torch.float32, device=tex.device)
        pyr[:tex.numel()].copy_(tex.reshape(-1))
        L.call('texmip_build', pyr, bt, F, C, len(sizes), _hw(sizes))
        ctx.meta = (tuple(tex.shape), sizes, F)
        return pyr

    @staticmethod
    def backward(ctx, g_pyr):
        shape, sizes, F = ctx.meta
        g_tex = torch.empty(shape, dtype=torch.float32, device=g_pyr.device)
        L.call('texmip_bwd', g_pyr.contiguous(), g_tex, shape[0], F, shape[-1], len(sizes), _hw(sizes))
        return g_tex, None, None


class _LookupFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pyr, uv, uv_da, bias, meta):
        bt, C, sizes, filt, bnd = meta
        nb, h, w = uv.shape[:3]
        out = torch.empty(nb, h, w, C, dtype=torch.float32, device=uv.device)
        L.call('texlookup_fwd', pyr, bt, C, len(sizes), _hw(sizes), uv, uv_da, bias, nb, h, w, filt, bnd, out)
        ctx.save_for_backward(pyr, uv, uv_da, bias)
        ctx.meta = meta
        return out

    @staticmethod
    def backward(ctx, g_out):
        pyr, uv, uv_da, bias = ctx.saved_tensors
        bt, C, sizes, filt, bnd = ctx.meta
        nb, h, w = uv.shape[:3]
        need = ctx.needs_input_grad
        d_pyr = L.zeros_like(pyr) if need[0] else None
        d_uv = torch.empty_like(uv) if need[1] else None
        d_da = torch.empty_like(uv_da) if need[2] else None
        d_bias = torch.empty_like(bias) if need[3] else None
        if d_pyr is not None or d_uv is not None or d_da is not None or d_bias is not None:
            L.call('texlookup_bwd', pyr, bt, C, len(sizes), _hw(sizes), uv, uv_da, bias, nb, h, w, filt, bnd, g_out.contiguous(), d_pyr, d_uv, d_da,
                   d_bias)
        return d_pyr, d_uv, d_da, d_bias, None


def _check_tex(tex, cube, what='tex'):
    if cube:
        if tex.dim() != 5 or tex.shape[1] != 6 or tex.shape[2] != tex.shape[3]:
            raise ValueError(f'd3h.texture: a cube map {what} must be [B|1, 6, H, H, C], got {tuple(tex.shape)}')
    elif tex.dim() != 4:
        raise ValueError(f'd3h.texture: {what} must be [B|1, H, W, C], got {tuple(tex.shape)}')


def texture_construct_mip(tex, max_mip_level=None, cube_mode=False):
    """the pyramid of `tex` (module docstring), for `mip=` of texture()"""
    _check_tex(tex, cube_mode)
    sizes = mip_sizes(tex.shape[-3], tex.shape[-2], max_mip_level)
    return TextureMip(_MipBuildFn.apply(tex, sizes, cube_mode), sizes, tex.shape[0], tex.shape[-1], cube_mode)


def _packed_levels(tex, mip, cube, max_mip_level):
    if isinstance(mip, TextureMip):
        if mip.cube != cube or mip.C != tex.shape[-1] or mip.bt != tex.shape[0] or mip.sizes[0] != (tex.shape[-3], tex.shape[-2]):
            raise ValueError('d3h.texture: the TextureMip was built from a texture of another shape or mode')
        sizes = mip.sizes if max_mip_level is None else mip.sizes[:max_mip_level + 1]
        return mip.pyr, sizes
    if mip is None:
        sizes = mip_sizes(tex.shape[-3], tex.shape[-2], max_mip_level)
        return _MipBuildFn.apply(tex, sizes, cube), sizes
    levels = [tex] + [m if m.dim() == tex.dim() else m[None] for m in mip]
    if max_mip_level is not None:
        levels = levels[:max_mip_level + 1]
    if len(levels) > MAX_LEVELS:
        raise ValueError(f'd3h.texture: at most {MAX_LEVELS} levels')
    for i, m in enumerate(levels[1:]):
        _check_tex(m, cube, f'mip[{i}]')
        if m.shape[0] != tex.shape[0] or m.shape[-1] != tex.shape[-1]:
            raise ValueError(f'd3h.texture: mip[{i}] {tuple(m.shape)} does not match the batch / channels of tex {tuple(tex.shape)}')
    return torch.cat([m.contiguous().float().reshape(-1) for m in levels]), [(m.shape[-3], m.shape[-2]) for m in levels]


def texture(tex, uv, uv_da=None, mip_level_bias=None, mip=None, filter_mode='auto', boundary_mode='wrap', max_mip_level=None):
    """nvdiffrast.texture (module docstring): [B, h, w, C]"""
    if filter_mode == 'auto':
        filter_mode = 'linear-mipmap-linear' if (uv_da is not None or mip_level_bias is not None) else 'linear'
    if filter_mode not in FILTERS:
        raise ValueError(f'd3h.texture: unknown filter_mode {filter_mode!r} (one of {sorted(FILTERS)} or "auto")')
    if boundary_mode not in BOUNDARIES:
        raise ValueError(f'd3h.texture: unknown boundary_mode {boundary_mode!r} (one of {sorted(BOUNDARIES)})')
    cube = boundary_mode == 'cube'
    mipmapped = filter_mode.startswith('linear-mipmap')
    _check_tex(tex, cube)
    if uv.dim() != 4 or uv.shape[-1] != (3 if cube else 2):
        raise ValueError(f'd3h.texture: uv must be [B, h, w, {3 if cube else 2}], got {tuple(uv.shape)}')
    nb = uv.shape[0]
    if tex.shape[0] not in (1, nb):
        raise ValueError(f'd3h.texture: the texture batch {tex.shape[0]} is neither 1 nor the lookup batch {nb}')
    if mipmapped:
        if cube and uv_da is not None:
            raise NotImplementedError('d3h.texture: cube maps take their mip level from mip_level_bias only; uv_da with boundary_mode="cube" '
                                      'is not implemented')
        if uv_da is None and mip_level_bias is None:
            raise ValueError(f'd3h.texture: filter_mode={filter_mode!r} needs uv_da or mip_level_bias')
        if uv_da is not None and tuple(uv_da.shape) != tuple(uv.shape[:3]) + (4,):
            raise ValueError(f'd3h.texture: uv_da must be [B, h, w, 4], got {tuple(uv_da.shape)}')
        if mip_level_bias is not None and tuple(mip_level_bias.shape) != tuple(uv.shape[:3]):
            raise ValueError(f'd3h.texture: mip_level_bias must be [B, h, w], got {tuple(mip_level_bias.shape)}')
        pyr, sizes = _packed_levels(tex, mip, cube, max_mip_level)
    else:
        uv_da = mip_level_bias = None
        pyr, sizes = tex.contiguous().float().reshape(-1), [(tex.shape[-3], tex.shape[-2])]
    f32 = (lambda t: None if t is None else t.contiguous().float())
    meta = (tex.shape[0], tex.shape[-1], sizes, FILTERS[filter_mode], BOUNDARIES[boundary_mode])
    return _LookupFn.apply(pyr, f32(uv), f32(uv_da), f32(mip_level_bias), meta)
