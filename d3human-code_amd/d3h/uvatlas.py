"""Host side of csrc/uvatlas.hip: the triangle-pair UV atlas of the textured-mesh export, the position bake into it, and the 2 x 2 mip op
of render/texture.py (the reference's xatlas.parametrize + render_uv + dilation, train.py:198-246, and texture2d_mip, render/texture.py:20-30).

    make_atlas(v_pos [V,3], t_pos_idx [F,3], resolution) -> Atlas(uvs [3F,2], t_tex_idx [F,3] int64, vmapping [3F], rot [F] uint8, s, nx, ny, resolution)
    bake_positions(atlas, v_pos, t_pos_idx) -> pos [1,H,W,3], owned [1,H,W,1], inside [1,H,W,1], tri [1,H,W] int32 (-1 = unowned)
    mip2x2(x [N,H,W,C]) -> [N,H/2,W/2,C], differentiable with the reference's gradient rule

The layout is closed-form (csrc/uvatlas.hip states it): two triangles per square cell of s texels, s the largest integer with
floor(W/s) * floor(H/s) >= ceil(F/2); no charts, no packing, no iteration, no host read-back.  Every face gets three uv vertices of its own, so
`vmapping` is just the flattened face list.  What the layout buys: a bilinear lookup at level 0 anywhere on the surface reads only texels
baked from the triangle the point lies on -- no seams, no dilation.  Its two limits:
  * texel efficiency is (s - 4)^2 / s^2 of each cell (a 2-texel gutter around every half cell);
  * mip levels above 0 average across triangles, so the baked maps are for level-0 bilinear use."""
import math
from collections import namedtuple

import torch

from . import _lib as L

Atlas = namedtuple('Atlas', 'uvs t_tex_idx vmapping rot s nx ny resolution')

MIN_CELL = 5


def _resolution(resolution):
    if isinstance(resolution, int):
        return int(resolution), int(resolution)
    H, W = (int(v) for v in resolution)
    return H, W


def cell_size(F, H, W):
    """-> (s, nx, ny): the largest s with (W // s) * (H // s) >= ceil(F / 2) (an empty mesh: one cell row of the shorter side); 0 if none"""
    cells = (F + 1) // 2
    top = min(H, W) if cells == 0 else min(H, W, math.isqrt(H * W // cells))      # (W // s)(H // s) <= W H / s^2: nothing above this can fit
    for s in range(top, 0, -1):
        if (W // s) * (H // s) >= cells:
            return s, W // s, H // s
    return 0, 0, 0


def _faces(t_pos_idx):
    if t_pos_idx.dim() != 2 or t_pos_idx.shape[1] != 3 or t_pos_idx.dtype not in (torch.int32, torch.int64):
        raise RuntimeError(f'uvatlas: expected t_pos_idx [F,3] int32 or int64, got {tuple(t_pos_idx.shape)} {t_pos_idx.dtype}')
    return t_pos_idx.contiguous()


def _verts(v_pos):
    if v_pos.dim() == 3:                     # a batch of posed frames: the first one
        v_pos = v_pos[0]
    if v_pos.dim() != 2 or v_pos.shape[1] != 3:
        raise RuntimeError(f'uvatlas: expected v_pos [V,3], got {tuple(v_pos.shape)}')
    return v_pos.detach().float().contiguous()


def make_atlas(v_pos, t_pos_idx, resolution):
    H, W = _resolution(resolution)
    if H < 1 or W < 1:
        raise ValueError(f'uvatlas: resolution must be positive, got {(H, W)}')
    v, t = _verts(v_pos), _faces(t_pos_idx)
    F = int(t.shape[0])
    s, nx, ny = cell_size(F, H, W)
    if s < MIN_CELL:
        need = MIN_CELL * (math.isqrt(max((F + 1) // 2 - 1, 0)) + 1)      # 5 ceil(sqrt(ceil(F / 2))), one cell for an empty mesh
        raise ValueError(f'uvatlas: a {H} x {W} texture is too small for {F} triangles (cells of {s} texels, {MIN_CELL} needed); '
                         f'the smallest square resolution that works is {need}')
    dev = v.device
    uvs = torch.empty(3 * F, 2, dtype=torch.float32, device=dev)
    t_tex_idx = torch.empty(F, 3, dtype=torch.int64, device=dev)
    rot = torch.empty(F, dtype=torch.uint8, device=dev)
    L.call('uvatlas_layout', v, v.shape[0], t, t.dtype == torch.int64, F, s, nx, H, W, uvs, t_tex_idx, rot)
    return Atlas(uvs, t_tex_idx, t_pos_idx.reshape(-1), rot, s, nx, ny, (H, W))


def bake_positions(atlas, v_pos, t_pos_idx):
    H, W = atlas.resolution
    v, t = _verts(v_pos), _faces(t_pos_idx)
    F = int(t.shape[0])
    if F != atlas.rot.shape[0]:
        raise RuntimeError(f'uvatlas: the atlas was made for {atlas.rot.shape[0]} triangles, got {F}')
    dev = v.device
    pos = torch.empty(1, H, W, 3, dtype=torch.float32, device=dev)
    owned, inside = (torch.empty(1, H, W, 1, dtype=torch.float32, device=dev) for _ in range(2))
    tri = torch.empty(1, H, W, dtype=torch.int32, device=dev)
    L.call('uvatlas_bake', v, v.shape[0], t, t.dtype == torch.int64, F, atlas.rot.contiguous(), atlas.s, atlas.nx, atlas.ny, H, W, pos, owned, inside,
           tri)
    return pos, owned, inside, tri


def _check_mip_input(x, what):
    if x.dim() != 4 or x.shape[3] < 1:
        raise RuntimeError(f'{what}: expected [N,H,W,C] with C >= 1, got {tuple(x.shape)}')


def mip2x2_fwd(x):
    """the 2 x 2 mean of an NHWC image with even H and W (no autograd: see mip2x2)"""
    _check_mip_input(x, 'mip2x2')
    N, H, W, C = x.shape
    if H < 2 or W < 2 or H % 2 or W % 2:
        raise ValueError(f"mip2x2: H and W must be even and at least 2, got {(H, W)} (the reference's gradient has the wrong shape there)")
    x = x.detach().float().contiguous()
    y = torch.empty(N, H // 2, W // 2, C, dtype=torch.float32, device=x.device)
    L.call('mip2x2_fwd', x, N, H // 2, W // 2, C, y)
    return y


def mip2x2_bwd(dy):
    """the gradient rule of the reference's texture2d_mip: the bilinear x2 upsample (texel centres, border clamped) of 0.25 dy -- not the
    adjoint of the mean"""
    _check_mip_input(dy, 'mip2x2_bwd')
    N, h, w, C = dy.shape
    dy = dy.detach().float().contiguous()
    dx = torch.empty(N, 2 * h, 2 * w, C, dtype=torch.float32, device=dy.device)
    L.call('mip2x2_bwd', dy, N, h, w, C, dx)
    return dx


class _Mip2x2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return mip2x2_fwd(x)

    @staticmethod
    def backward(ctx, dy):
        return mip2x2_bwd(dy)


def mip2x2(x):
    """mip2x2_fwd, differentiable with mip2x2_bwd as its gradient"""
    return _Mip2x2.apply(x)
