"""Host side of csrc/texmat.hip: the per-pixel material lookup of a textured mesh, the hot path of fitting texture maps on a fixed mesh.

    lookup(rast [B,H,W,4], v_tex [Vt,2], t_tex_idx32 [F,3] int32, maps, boundary='wrap') -> one image [B,H,W,C_i] per map

`maps`: 1-3 tensors [1,H_i,W_i,C_i] (C_i <= 4), each of its own resolution (a 1 x 1 map is a constant).  Per pixel the texel coordinate is
interpolated from the three v_tex rows of the pixel's triangle (the barycentric convention of d3h.raster.interpolate) and every map is read
with one level-0 bilinear lookup in the conventions of d3h/texture.py ('wrap' or 'clamp'); an empty pixel gets zeros.  Differentiable in
the maps only (fp32 atomics into zero-filled buffers, only for the maps that require a gradient): `rast` and `v_tex` get none -- a caller
that needs uv or shape gradients composes d3h.raster.interpolate with d3h.texture.texture instead, which gives the same values."""
import ctypes

import torch

from . import _lib as L

BOUNDARIES = {'wrap': 0, 'clamp': 1}
MAX_MAPS = 3
MAX_CHANNELS = 4


def _hwc(maps):
    flat = [int(v) for m in maps for v in m.shape[1:4]]
    return (ctypes.c_int * len(flat))(*flat)


class _LookupFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rast, v_tex, tri, bnd, *maps):
        B, H, W = rast.shape[:3]
        npix, F = B * H * W, tri.shape[0]
        new = torch.zeros if F == 0 else torch.empty                       # F == 0 launches nothing
        outs = [new(B, H, W, m.shape[-1], dtype=torch.float32, device=rast.device) for m in maps]
        L.call('texmat_fwd', rast, v_tex, v_tex.shape[0], tri, F, npix, len(maps), L.ptr_array(maps), _hwc(maps), bnd, L.ptr_array(outs))
        ctx.save_for_backward(rast, v_tex, tri, *maps)
        ctx.bnd = bnd
        return tuple(outs)

    @staticmethod
    def backward(ctx, *g_outs):
        rast, v_tex, tri, *maps = ctx.saved_tensors
        need = ctx.needs_input_grad[4:]
        B, H, W = rast.shape[:3]
        grads = [L.zeros_like(m) if n and g is not None else None for m, n, g in zip(maps, need, g_outs)]
        g_in = [None if d is None else g.contiguous().float() for d, g in zip(grads, g_outs)]
        if any(d is not None for d in grads):
            L.call('texmat_bwd', rast, v_tex, v_tex.shape[0], tri, tri.shape[0], B * H * W, len(maps), L.ptr_array(maps), _hwc(maps), ctx.bnd, L.ptr_array(g_in),
                   L.ptr_array(grads))
        return (None, None, None, None) + tuple(grads)


def lookup(rast, v_tex, t_tex_idx32, maps, boundary='wrap'):
    """module docstring"""
    maps = list(maps)
    if boundary not in BOUNDARIES:
        raise ValueError(f'd3h.texmat: unknown boundary {boundary!r} (one of {sorted(BOUNDARIES)})')
    if not 1 <= len(maps) <= MAX_MAPS:
        raise ValueError(f'd3h.texmat: 1 to {MAX_MAPS} maps, got {len(maps)}')
    for m in maps:
        if m.dim() != 4 or m.shape[0] != 1 or not 1 <= m.shape[-1] <= MAX_CHANNELS or m.shape[1] < 1 or m.shape[2] < 1:
            raise ValueError(f'd3h.texmat: a map must be [1,H,W,C] with C <= {MAX_CHANNELS}, got {tuple(m.shape)}')
    if rast.dim() != 4 or rast.shape[-1] != 4:
        raise ValueError(f'd3h.texmat: rast must be [B,H,W,4], got {tuple(rast.shape)}')
    if v_tex.dim() != 2 or v_tex.shape[-1] != 2:
        raise ValueError(f'd3h.texmat: v_tex must be [Vt,2], got {tuple(v_tex.shape)}')
    if t_tex_idx32.dim() != 2 or t_tex_idx32.shape[-1] != 3 or t_tex_idx32.dtype != torch.int32:
        raise ValueError(f'd3h.texmat: t_tex_idx32 must be [F,3] int32, got {tuple(t_tex_idx32.shape)} {t_tex_idx32.dtype}')
    if rast.requires_grad or v_tex.requires_grad:
        raise ValueError('d3h.texmat: the fused lookup gives no gradient to rast or v_tex; compose interpolate + texture for those')
    return list(_LookupFn.apply(rast.detach().float().contiguous(), v_tex.detach().float().contiguous(), t_tex_idx32.contiguous(), BOUNDARIES[boundary],
                                *[m.float().contiguous() for m in maps]))
