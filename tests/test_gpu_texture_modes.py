"""d3h.texture (csrc/texture.hip) on the MI355X against the float64 restatement of test_texture_modes.py, at working sizes: 1024^2 lookups
into 2048^2 and 1080^2 textures and a 6 x 256^2 cube map.

Both sides read the same float32 inputs.  The kernel forms texel coordinates in float32 (an ulp of u * 2048 is 1.2e-4 texel), hence
RTOL = 1e-4 on values.  A few lookups land within that rounding of a texel edge or a mip-level boundary, where nearest filtering, the level
pick and the uv / uv_da / bias gradients jump: `close` lets a fraction BAD = 1e-3 of the elements differ, everything else within tolerance."""
import math

import pytest
import torch

import test_texture_modes as TM

BAD = 1e-3
RTOL = 1e-4


def _case_2d(gen, size, C, bt=1, B=1, res=1024):
    tex, uv, _, bias = TM.make_case(gen, bt, B, size, size, C, res, res, uv_lo=-0.2, uv_hi=1.2, with_bias=True)
    # footprints spread over every level: |J| ~ 2^U / size, U uniform in [-1, log2(size) + 1]
    U = torch.rand(B, res, res, 1, generator=gen, dtype=torch.float64) * (math.log2(size) + 2) - 1
    da = torch.randn(B, res, res, 4, generator=gen, dtype=torch.float64) * torch.exp2(U) / size
    return tex, uv, da, bias


@pytest.mark.gpu
@pytest.mark.parametrize('filter_mode', TM.FILTERS)
@pytest.mark.parametrize('boundary_mode', ('wrap', 'clamp', 'zero'))
def test_gpu_modes_2048(gpu, filter_mode, boundary_mode):
    gen = torch.Generator().manual_seed(100 + TM.FILTERS.index(filter_mode))
    tex, uv, da, bias = _case_2d(gen, 2048, 4)
    use_bias = boundary_mode == 'zero'
    TM.run_compare(gpu, tex, uv, da, bias if use_bias else None, filter_mode, boundary_mode, gen=gen, rtol=RTOL, grtol=5e-4, bad_frac=BAD)


@pytest.mark.gpu
def test_gpu_1080_broadcast(gpu):
    """a non-power-of-two texture (pyramid 1080 .. 135), three channels, broadcast over a batch of two lookups"""
    gen = torch.Generator().manual_seed(7)
    tex, uv, da, bias = _case_2d(gen, 1080, 3, bt=1, B=2, res=512)
    for filt in ('linear-mipmap-linear', 'linear-mipmap-nearest'):
        TM.run_compare(gpu, tex, uv, da, bias, filt, 'wrap', gen=gen, rtol=RTOL, grtol=5e-4, bad_frac=BAD)
    TM.run_compare(gpu, tex, uv, da, None, 'linear-mipmap-linear', 'clamp', max_mip_level=2, gen=gen, rtol=RTOL, grtol=5e-4, bad_frac=BAD)


@pytest.mark.gpu
@pytest.mark.parametrize('filter_mode', TM.FILTERS)
def test_gpu_cube_256(gpu, filter_mode):
    gen = torch.Generator().manual_seed(21)
    tex, uv, _, bias = TM.make_case(gen, 1, 1, 256, 256, 4, 1024, 1024, cube=True, with_bias='mipmap' in filter_mode)
    if bias is not None:
        bias.mul_(3.0)                                          # levels 0 .. 8
    TM.run_compare(gpu, tex, uv, None, bias, filter_mode, 'cube', gen=gen, rtol=RTOL, grtol=5e-4, bad_frac=BAD)


@pytest.mark.gpu
def test_gpu_latlong_cube_round_trip(gpu):
    """render/util.py: a smooth 512 x 1024 lat-long map -> 6 x 256^2 cube (wrap lookups) -> lat-long (cube lookups): within 5e-3
    (two bilinear resamplings of a field whose curvature over a texel is ~1e-5; the bound is set by the poles' lat-long sampling)"""
    from render import util
    H = 512
    v, u = torch.meshgrid((torch.arange(H, device=gpu) + 0.5) / H, (torch.arange(2 * H, device=gpu) + 0.5) / (2 * H), indexing='ij')
    th, ph = v * math.pi, (u - 0.5) * 2 * math.pi
    d = torch.stack((torch.sin(th) * torch.sin(ph), torch.cos(th), -torch.sin(th) * torch.cos(ph)), dim=-1)
    L = torch.stack((0.5 + 0.3 * d[..., 0], 0.5 + 0.3 * d[..., 1] * d[..., 2], 0.4 + 0.2 * d[..., 2] ** 2), dim=-1).float().contiguous()
    cube = util.latlong_to_cubemap(L, [256, 256])
    back = util.cubemap_to_latlong(cube, [H, 2 * H])
    err = (back - L).abs().max().item()
    assert err < 5e-3, err


@pytest.mark.gpu
def test_gpu_texture2d_flow(gpu):
    """render/texture.py Texture2D.sample: a list pyramid, uv and uv_da from rasterize + interpolate of a tilted quad; the gradient reaches
    the base and every level, and matches the restatement"""
    from d3h import raster
    import nvdiffrast.torch as dr
    gen = torch.Generator().manual_seed(31)
    wf = 400.0                                            # a floor receding to the horizon: footprints from ~1 texel to the whole texture
    pos = torch.tensor([[-0.9, -0.9, 0.5, 1.0], [0.9, -0.9, 0.5, 1.0], [-0.9 * wf, 0.99 * wf, 0.9 * wf, wf], [0.9 * wf, 0.99 * wf, 0.9 * wf, wf]],
                       device=gpu)[None]
    tri = torch.tensor([[0, 1, 2], [2, 1, 3]], dtype=torch.int32, device=gpu)
    uv_attr = torch.tensor([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0], [1.0, 1.0]], device=gpu)
    rast, db = raster.rasterize(pos, tri, (512, 512))
    texc, texd = dr.interpolate(uv_attr, rast, tri, rast_db=db, diff_attrs='all')
    assert texd is not None and float(texd.abs().max()) > 0
    base = torch.rand(1, 512, 512, 3, generator=gen, dtype=torch.float64)
    mips = [torch.rand(1, 512 >> k, 512 >> k, 3, generator=gen, dtype=torch.float64) for k in range(1, 9)]
    _, mk = TM.run_compare(gpu, base, texc.detach().double().cpu(), texd.detach().double().cpu(), None, 'linear-mipmap-linear', 'wrap',
                           mip=mips, gen=gen, grads=('tex',), rtol=RTOL, grtol=5e-4, bad_frac=BAD)
    reached = [float(m.grad.abs().max()) > 0 for m in mk]
    assert all(reached), reached
    # the same through the shim as Texture2D.sample calls it (positional uv_da, mip = the list)
    levels = [base.float().to(gpu).requires_grad_(True)] + [m.float().to(gpu).requires_grad_(True) for m in mips]
    out = dr.texture(levels[0], texc, texd, mip=levels[1:], filter_mode='linear-mipmap-linear')
    out.sum().backward()
    assert all(t.grad is not None for t in levels)
    assert [float(t.grad.abs().max()) > 0 for t in levels[1:]] == reached


@pytest.mark.gpu
def test_gpu_shim_linear_clamp_is_raster_texture(gpu):
    """explicit linear / clamp calls without a uv gradient stay on d3h.raster.texture, bit for bit"""
    import nvdiffrast.torch as dr
    from d3h import raster
    gen = torch.Generator().manual_seed(41)
    tex = torch.rand(2, 300, 200, 3, generator=gen).to(gpu).requires_grad_(True)
    uv = (torch.rand(2, 256, 256, 2, generator=gen) * 1.2 - 0.1).to(gpu)
    a = dr.texture(tex, uv, filter_mode='linear', boundary_mode='clamp')
    b = raster.texture(tex, uv, filter_mode='linear', boundary_mode='clamp')
    assert torch.equal(a, b)
    ga, = torch.autograd.grad(a.sum(), tex)
    assert ga.shape == tex.shape
