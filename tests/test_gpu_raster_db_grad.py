"""Differentiable pixel derivatives on the MI355X against the float64 restatement of test_raster_db_grad.py, at working sizes: two 1024^2
frames of the synth marching-tets body mesh (12.6 k faces) and of a ~100 k-triangle random mesh, one 1080^2 frame, the attribute derivatives of those
renders, and the rasterize -> interpolate -> mip-mapped texture chain of a receding quad.  The restatement runs in float64 on the same device
at the kernel's own triangle ids.

The bars, as relative-to-max-norm errors (`close` of test_texture_modes.py):
  - rasterize d_pos, RTOL_POS = 1e-3 with a bad fraction BAD_POS = 1e-3 of the position entries.  The kernel forms edge functions, S and
    1/S in float32: a pixel centre next to an edge of a thin triangle has a few correct bits in a_k, and db = O(1/S^2) amplifies that, so a
    few vertices of slivers differ by more than float32 rounding of the sum; everything else agrees to ~1e-5 (the host emulation, which runs
    the same float32 arithmetic, meets 2e-4 with no bad entry on meshes without slivers).
  - interpolate RTOL_INTERP = 1e-4: one product per term, but d_attr is an fp32 atomic sum over up to 10^6 pixels.
  - the texture chain: output and d_tex as test_gpu_texture_modes.py (1e-4 / 5e-4, a bad fraction of 1e-3 for lookups within float32 rounding
    of a texel edge or a level boundary); d_pos and d_uv_attr, four vertices summing 10^6 pixels, RTOL_CHAIN = 2e-3.  The texture is smooth,
    so a pixel whose texel or level pick flips between float32 and float64 changes its term by a second difference of the texture, not by
    a first one."""
import math

import pytest
import torch

import test_raster_db_grad as R

RTOL_POS, BAD_POS = 1e-3, 1e-3
RTOL_INTERP = 1e-4
RTOL_CHAIN = 2e-3


def _body_clip(res, B):
    """the synth body mesh (marching tets of synth.body_sdf on a 72^3 Kuhn grid: 12.6 k faces) in B slightly shifted placements"""
    from d3h import mtets, synth
    v, t = (torch.from_numpy(a) for a in synth.kuhn_grid(72))
    o = mtets.marching_tets(v.cuda(), synth.body_sdf(v).cuda(), torch.ones(v.shape[0]).cuda(), t.cuda())
    verts, tri = o['verts'], o['faces32']
    _, mvp, _ = synth.camera(res)
    offs = torch.tensor([[0.02 * b, 0.0, 0.0] for b in range(B)]).cuda()
    vh = torch.cat([verts[None] + offs[:, None], torch.ones(B, verts.shape[0], 1).cuda()], -1)
    return (vh @ torch.from_numpy(mvp).cuda().T).contiguous(), tri


@pytest.mark.gpu
def test_gpu_raster_db_body_1024(gpu):
    gen = torch.Generator().manual_seed(1)
    clip, tri = _body_clip(1024, 2)
    assert tri.shape[0] > 10_000, tri.shape
    R.check_raster(gpu, clip, tri, 1024, 1024, gen=gen, rtol=RTOL_POS, bad_frac=BAD_POS, min_cov=50_000)


@pytest.mark.gpu
def test_gpu_raster_db_random_100k(gpu):
    gen = torch.Generator().manual_seed(2)
    pos, tri = R.random_mesh(gen, 100_000, B=2, size=0.012)
    pos, tri = pos.cuda(), tri.cuda()
    R.check_raster(gpu, pos, tri, 1024, 1024, gen=gen, rtol=RTOL_POS, bad_frac=BAD_POS, min_cov=500_000)
    R.check_raster(gpu, pos[:1].contiguous(), tri, 1024, 1024, nb=2, gen=gen, rtol=RTOL_POS, bad_frac=BAD_POS, min_cov=500_000)   # broadcast


@pytest.mark.gpu
def test_gpu_raster_db_1080(gpu):
    gen = torch.Generator().manual_seed(3)
    clip, tri = _body_clip(1080, 1)
    R.check_raster(gpu, clip, tri, 1080, 1080, gen=gen, rtol=RTOL_POS, bad_frac=BAD_POS, min_cov=30_000)


@pytest.mark.gpu
@pytest.mark.parametrize('diff_attrs', ['all', [2, 0]])
def test_gpu_interpolate_da_body(gpu, diff_attrs):
    from d3h import raster
    gen = torch.Generator().manual_seed(4)
    clip, tri = _body_clip(1024, 2)
    rast, db = raster.rasterize(clip, tri, (1024, 1024))
    nv, A, B = clip.shape[1], 5, 2
    nd = 2 * (A if diff_attrs == 'all' else len(diff_attrs))
    for bcast in (False, True):
        attr = torch.randn(1 if bcast else B, nv, A, generator=gen, dtype=torch.float64).cuda()
        G_out = torch.randn(B, 1024, 1024, A, generator=gen, dtype=torch.float64).cuda()
        G_da = torch.randn(B, 1024, 1024, nd, generator=gen, dtype=torch.float64).cuda()
        g = R.check_interp(gpu, rast, db, tri, attr, diff_attrs, G_out, G_da, rtol=RTOL_INTERP)
        assert float(g[2].abs().max()) > 0
        g = R.check_interp(gpu, rast, db, tri, attr, diff_attrs, None, G_da, rtol=RTOL_INTERP)
        assert float(g[1].abs().max()) == 0
        R.check_interp(gpu, rast, db, tri, attr, diff_attrs, G_out, None, rtol=RTOL_INTERP)
    # an index buffer of its own (a uv chart's vertices)
    tri2 = torch.randint(0, 4000, tuple(tri.shape), generator=gen, dtype=torch.int32).cuda()
    attr2 = torch.randn(1, 4000, 3, generator=gen, dtype=torch.float64).cuda()
    G_da = torch.randn(B, 1024, 1024, 4, generator=gen, dtype=torch.float64).cuda()
    R.check_interp(gpu, rast, db, tri2, attr2, [1, 2], torch.randn(B, 1024, 1024, 3, generator=gen, dtype=torch.float64).cuda(), G_da,
                   rtol=RTOL_INTERP)


@pytest.mark.gpu
def test_gpu_texture_chain_1024(gpu):
    """dr.rasterize -> dr.interpolate(diff_attrs='all') -> dr.texture('linear-mipmap-linear', 'wrap') of a receding quad at 1024^2 into a
    smooth 1024^2 texture: the gradient through uv_da and db reaches pos and uv_attr, and matches the restatement chain"""
    gen = torch.Generator().manual_seed(5)
    pos, tri, uv_attr = R.receding_quad(gpu)
    y, x = torch.meshgrid((torch.arange(1024, dtype=torch.float64) + 0.5) / 1024, (torch.arange(1024, dtype=torch.float64) + 0.5) / 1024,
                          indexing='ij')
    tex = torch.stack([0.5 + 0.4 * torch.sin(2 * math.pi * (3 * x + y)), 0.5 + 0.3 * torch.cos(2 * math.pi * (2 * y - x)),
                       0.5 + 0.2 * torch.sin(2 * math.pi * 5 * x) * torch.cos(2 * math.pi * 4 * y)], -1)[None]
    g = R.check_chain(gpu, pos, tri, uv_attr, tex, (1024, 1024), gen, rtol=1e-4, bad_frac=1e-3, grtol=RTOL_CHAIN, tex_grtol=5e-4)
    assert float(g[0].abs().max()) > 0 and float(g[1].abs().max()) > 0


@pytest.mark.gpu
def test_gpu_grad_db_false_is_the_existing_path(gpu):
    """grad_db False, and grad_db True with db unused: the same single d3h_rasterize_bwd launch and no new entry point, rast and db bit for bit, d_pos up to the order of its atomics (fp32 atomicAdd of per-run sums from different waves)"""
    import nvdiffrast.torch as dr
    from d3h import _lib as L, raster
    gen = torch.Generator().manual_seed(6)
    clip, tri = _body_clip(1024, 2)
    G1 = torch.randn(2, 1024, 1024, 4, generator=gen).cuda()
    names = ('d3h_rasterize_bwd', 'd3h_rasterize_bwd_db', 'd3h_interpolate_bwd_da')
    outs = []
    for how in ('raster', 'shim', 'peeler', 'grad_db_unused'):
        cnt = R._Counting(L.lib(), names)
        L._lib = cnt
        try:
            p = clip.clone().requires_grad_(True)
            if how == 'raster':
                rast, db = raster.rasterize(p, tri, (1024, 1024))
            elif how == 'shim':
                rast, db = dr.rasterize(None, p, tri, (1024, 1024), grad_db=False)
            elif how == 'peeler':
                with dr.DepthPeeler(None, p, tri, (1024, 1024), grad_db=False) as peeler:
                    rast, db = peeler.rasterize_next_layer()
            else:
                rast, db = raster.rasterize(p, tri, (1024, 1024), grad_db=True)
            g, = torch.autograd.grad((rast * G1).sum(), p)
        finally:
            L._lib = cnt._l
        assert cnt.calls == {'d3h_rasterize_bwd': 1, 'd3h_rasterize_bwd_db': 0, 'd3h_interpolate_bwd_da': 0}, (how, cnt.calls)
        outs.append((rast.detach(), db.detach(), g))
    r0, d0, g0 = outs[0]
    for r, d, g in outs[1:]:
        assert torch.equal(r, r0) and torch.equal(d, d0)
        assert float((g - g0).abs().max()) <= 1e-5 * float(g0.abs().max()), float((g - g0).abs().max())
