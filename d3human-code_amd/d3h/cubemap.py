"""Host side of csrc/cubemap.hip: diffuse_cubemap / specular_cubemap of render.renderutils (autograd).

Cached on the host: per (N, device) the texel table {direction, pixel_area} the kernels sweep and the bounding cones of its 16 x 16 patches
(which let a workgroup skip the patches its filter cannot reach); per (N, roughness, cutoff) the cone's
cos(theta) cutoff -- 10^6 samples of the GGX NDF over [0, pi/2], cut at the first sample where the running sum reaches `cutoff` of the total
(numpy, float64: the recipe of the reference, render/renderutils/ops.py:431-446, without its bounds table).  The backward of both filters is a
gather over the same table: no atomics, bit-reproducible."""
import numpy as np
import torch

from . import _lib as L

_TABLES = {}
_CUTOFFS = {}
PATCH = 16                  # CM_P of csrc/cubemap.hip


def _face_dir(side, fx, fy):
    """the (unnormalised) direction through the point (fx, fy) in [-1, 1]^2 of face `side` (+x, -x, +y, -y, +z, -z)"""
    one = np.ones_like(fx)
    return np.stack([(one, -fy, -fx), (-one, -fy, fx), (fx, one, fy), (fx, -one, -fy), (fx, -fy, one), (-fx, -fy, -one)][side], -1)


def patch_cones(N):
    """[6 ceil(N / 16)^2, 4] float64: for every 16 x 16 patch of a face (row-major inside a face, faces in order) the direction through the
    centre of its rectangle and the largest angle from it to the rectangle's corners.  The set of points of a plane within a given angle
    (< 90 degrees) of an axis is convex, so the corners bound the whole rectangle, and with it every texel direction of the patch."""
    ppf = -(-N // PATCH)
    out = []
    for side in range(6):
        for py in range(ppf):
            for px in range(ppf):
                x = np.array([px * PATCH, min(N, (px + 1) * PATCH)], np.float64) * 2.0 / N - 1.0
                y = np.array([py * PATCH, min(N, (py + 1) * PATCH)], np.float64) * 2.0 / N - 1.0
                unit = lambda v: v / np.linalg.norm(v, axis=-1, keepdims=True)
                axis = unit(_face_dir(side, x.mean(keepdims=True), y.mean(keepdims=True)))[0]
                cy, cx = np.meshgrid(y, x, indexing='ij')
                corners = unit(_face_dir(side, cx.reshape(-1), cy.reshape(-1)))
                out.append([*axis, float(np.arccos(np.clip(corners @ axis, -1.0, 1.0)).max())])
    return np.array(out, np.float64)


def texel_table(N, device):
    """([6 N^2, 4] float32: unit direction and pixel_area of every texel, order [side][y][x]; [patches, 4] float32: patch_cones(N))"""
    key = (int(N), str(device), L.emulated())
    t = _TABLES.get(key)
    if t is None:
        table = torch.empty(6 * N * N, 4, dtype=torch.float32, device=device)
        L.call('cubemap_table', N, table)
        t = _TABLES[key] = (table, torch.from_numpy(patch_cones(N)).float().to(device).contiguous())
    return t


def costheta_cutoff(N, roughness, cutoff):
    key = (int(N), float(roughness), float(cutoff))
    c = _CUTOFFS.get(key)
    if c is None:
        cos_t = np.cos(np.linspace(0.0, np.pi / 2.0, 1000000))
        a2 = float(roughness) ** 4
        d = (cos_t * a2 - cos_t) * cos_t + 1.0
        run = np.cumsum(a2 / (d * d * np.pi))
        c = _CUTOFFS[key] = float(cos_t[np.argmax(run >= run[-1] * cutoff)])
    return c


def _check(cubemap, what):
    if cubemap.dim() != 4 or cubemap.shape[0] != 6 or cubemap.shape[1] != cubemap.shape[2] or cubemap.shape[3] != 3 or cubemap.shape[1] < 1:
        raise RuntimeError(f'{what}: bad shape for the cubemap tensor: {tuple(cubemap.shape)} (expected [6, N, N, 3])')
    return int(cubemap.shape[1])


class _DiffuseFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cubemap):
        N = _check(cubemap, 'diffuse_cubemap')
        c = cubemap.contiguous().float()
        out = torch.empty_like(c)
        L.call('cubemap_diffuse', *texel_table(N, c.device), c, N, 0, out)
        ctx.N = N
        return out

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous().float()
        d = torch.empty_like(g)
        L.call('cubemap_diffuse', *texel_table(ctx.N, g.device), g, ctx.N, 1, d)
        return d


class _SpecularFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cubemap, roughness, cut):
        N = _check(cubemap, 'specular_cubemap')
        c = cubemap.contiguous().float()
        out = torch.empty_like(c)
        wsum = torch.empty(6 * N * N, dtype=torch.float32, device=c.device)
        L.call('cubemap_specular_fwd', *texel_table(N, c.device), c, N, roughness, cut, out, wsum)
        ctx.save_for_backward(wsum)            # depends on (N, roughness, cutoff) only, not on the cubemap
        ctx.meta = (N, float(roughness), float(cut))
        return out

    @staticmethod
    def backward(ctx, g):
        wsum, = ctx.saved_tensors
        N, roughness, cut = ctx.meta
        g = g.contiguous().float()
        d = torch.empty_like(g)
        L.call('cubemap_specular_bwd', *texel_table(N, g.device), g, wsum, N, roughness, cut, d)
        return d, None, None


def diffuse_cubemap(cubemap):
    """[6,N,N,3] -> [6,N,N,3]: out[p] = sum_q clamp(d_p . d_q, 0, 0.999) area(q) / 3.141592 cubemap[q] over all 6 N^2 texels"""
    return _DiffuseFn.apply(cubemap)


def specular_cubemap(cubemap, roughness, cutoff=0.99):
    """[6,N,N,3] -> [6,N,N,3]: the GGX-weighted mean of the texels inside the cone that holds `cutoff` of the lobe's energy"""
    N = _check(cubemap, 'specular_cubemap')
    return _SpecularFn.apply(cubemap, float(roughness), costheta_cutoff(N, roughness, cutoff))
