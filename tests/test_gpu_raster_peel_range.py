"""Depth peeling and range mode on the MI355X at working sizes, against the float32 restatement of test_raster_peel_range.py (every fragment
key of every pixel) and the float64 gradient restatement of test_raster_db_grad.py.  Scenes: the synth marching-tets body mesh (12.6 k faces)
and a ~100 k-triangle random mesh at 2 x 1024^2; the body mesh in four placements at 4 x 1024^2 in range mode.

Every peel loop stops at LAYER_CAP layers and asserts that the layer that ended it is empty.  The layer-by-layer ids may differ from the
restatement at a fraction BAD_IDS = 1e-4 of the covered pixels (the restatement runs numpy's float32 arithmetic; the kernel's is that of the
device); the gradient bars are test_gpu_raster_db_grad.py's."""
import numpy as np
import pytest
import torch

import test_gpu_raster_db_grad as G
import test_raster_db_grad as R
import test_raster_peel_range as P

BAD_IDS = 1e-4


def _peel_checked(pos, tri, H, W, ranges=None):
    """peel until empty; layer 0 equals rasterize bit for bit, no (pixel, id) pair appears twice, z/w does not decrease (one ulp), and the
    layers agree with the restatement -- per frame the count of all fragments and, layer by layer, the ids"""
    from d3h import raster
    layers = P.peel_all(pos, tri, H, W, ranges)
    r0, d0 = raster.rasterize(pos, tri, (H, W), ranges=ranges)
    assert torch.equal(layers[0][0], r0) and torch.equal(layers[0][1], d0)
    ids = torch.stack([r[..., 3] for r, _ in layers]).long()                 # [L, B, H, W]
    z = torch.stack([r[..., 2] for r, _ in layers])
    cov = ids > 0
    assert bool((cov[1:] <= cov[:-1]).all()), 'a pixel came back after an empty layer'
    both = cov[1:] & cov[:-1]
    zlo = torch.nextafter(z[:-1], torch.full_like(z[:-1], -float('inf')))
    assert bool((z[1:][both] >= zlo[both]).all()), 'z/w decreased from one layer to the next'
    srt, _ = ids.sort(0)
    assert not bool(((srt[1:] == srt[:-1]) & (srt[1:] > 0)).any()), 'a (pixel, id) pair in two layers'
    ref = P.ref_layers(pos.cpu().numpy(), tri.cpu().numpy(), H, W, None if ranges is None else ranges.numpy())
    got = ids.cpu().numpy()
    npix_cov = max(int(cov[0].sum()), 1)
    for b in range(got.shape[1]):
        n_got = int((got[:, b] > 0).sum())
        n_ref = int(sum((r[b] > 0).sum() for r in ref))
        assert abs(n_got - n_ref) <= BAD_IDS * npix_cov, (b, n_got, n_ref)
    nl = max(len(ref), got.shape[0])
    for k in range(nl):
        gk = got[k] if k < got.shape[0] else np.zeros_like(got[0])
        rk = ref[k] if k < len(ref) else np.zeros_like(gk)
        assert int((gk != rk).sum()) <= BAD_IDS * npix_cov, (k, int((gk != rk).sum()), npix_cov)
    return layers


def _layer_grads(gpu, pos, tri, H, W, gen, layers_to_check=(1, 2), min_cov=100):
    import nvdiffrast.torch as dr
    p = pos.clone().requires_grad_(True)
    with dr.DepthPeeler(None, p, tri, (H, W), grad_db=True) as peeler:
        layers = [peeler.rasterize_next_layer() for _ in range(max(layers_to_check) + 1)]
    B = pos.shape[0]
    for k in layers_to_check:
        rast, db = layers[k]
        assert int((rast[..., 3] > 0).sum()) >= min_cov, k
        G1 = torch.randn(B, H, W, 2, generator=gen, dtype=torch.float64)
        G2 = torch.randn(B, H, W, 4, generator=gen, dtype=torch.float64)
        loss = (db * G2.float().to(gpu)).sum() + (rast[..., :2] * G1.float().to(gpu)).sum()
        g, = torch.autograd.grad(loss, p, retain_graph=True)
        gr, dbr = R.ref_rast_grads(pos, tri, rast[..., 3].detach().long(), H, W, G1.to(gpu), G2.to(gpu))
        R.TM.close(db, dbr, G.RTOL_POS, f'layer {k} db', G.BAD_POS)
        R.TM.close(g, gr, G.RTOL_POS, f'layer {k} d_pos', G.BAD_POS)


@pytest.mark.gpu
def test_gpu_peel_body_1024(gpu):
    clip, tri = G._body_clip(1024, 2)
    assert tri.shape[0] > 10_000
    layers = _peel_checked(clip, tri, 1024, 1024)
    assert len(layers) >= 2, len(layers)
    # a closed surface seen from the front: two layers (layer 2 is empty), so the gradient check covers layer 1; test_gpu_peel_random_100k
    # covers layers 1 and 2
    _layer_grads(gpu, clip, tri, 1024, 1024, torch.Generator().manual_seed(11), layers_to_check=(1,))


@pytest.mark.gpu
def test_gpu_peel_random_100k(gpu):
    gen = torch.Generator().manual_seed(12)
    pos, tri = R.random_mesh(gen, 100_000, B=2, size=0.012)
    pos, tri = pos.cuda(), tri.cuda()
    layers = _peel_checked(pos, tri, 1024, 1024)
    assert len(layers) >= 4, len(layers)
    _layer_grads(gpu, pos, tri, 1024, 1024, gen)


@pytest.mark.gpu
def test_gpu_range_mode_body_4x1024(gpu):
    """the body mesh in four placements, one tri / pos, one range each: every frame is the instanced render with offset ids, bit for bit
    (rast, db, and the peeled layers 1 and 2); d_pos is the sum of the instanced gradients up to fp32 atomic order"""
    from d3h import raster
    gen = torch.Generator().manual_seed(13)
    clip, tri = G._body_clip(1024, 4)
    B, V = clip.shape[:2]
    F = tri.shape[0]
    pos2 = clip.reshape(-1, 4).contiguous()
    tri_all = torch.cat([tri + b * V for b in range(B)], 0).int().contiguous()
    ranges = torch.tensor([[b * F, F] for b in range(B)], dtype=torch.int32)
    G1 = torch.randn(B, 1024, 1024, 4, generator=gen).cuda()
    G2 = torch.randn(B, 1024, 1024, 4, generator=gen).cuda()
    p = pos2.clone().requires_grad_(True)
    rast, db = raster.rasterize(p, tri_all, (1024, 1024), grad_db=True, ranges=ranges)
    g, = torch.autograd.grad((rast * G1).sum() + (db * G2).sum(), p)
    ref = torch.zeros_like(pos2)
    prev_i = []
    for b in range(B):
        tb = tri_all[b * F:(b + 1) * F].contiguous()
        pb = pos2[None].clone().requires_grad_(True)
        rb, dbb = raster.rasterize(pb, tb, (1024, 1024), grad_db=True)
        ref += torch.autograd.grad((rb * G1[b]).sum() + (dbb * G2[b]).sum(), pb)[0][0]
        rb = rb.detach().clone()
        rb[..., 3] = torch.where(rb[..., 3] > 0, rb[..., 3] + b * F, rb[..., 3])
        assert torch.equal(rast[b].detach(), rb[0]) and torch.equal(db[b].detach(), dbb[0].detach()), b
        prev_i.append((pb.detach(), tb))
    R.TM.close(g, ref, 1e-5, 'range-mode d_pos')
    assert float(g.abs().max()) > 0
    # peeling in range mode: layers 1 and 2 of every frame equal the instanced layers with offset ids
    import nvdiffrast.torch as dr
    with dr.DepthPeeler(None, pos2, tri_all, (1024, 1024), ranges=ranges) as peeler:
        rl = [peeler.rasterize_next_layer()[0] for _ in range(3)]
    for b, (pb, tb) in enumerate(prev_i):
        with dr.DepthPeeler(None, pb, tb, (1024, 1024)) as peeler:
            il = [peeler.rasterize_next_layer()[0] for _ in range(3)]
        for k in (1, 2):
            r = il[k].clone()
            r[..., 3] = torch.where(r[..., 3] > 0, r[..., 3] + b * F, r[..., 3])
            assert torch.equal(rl[k][b], r[0]), (b, k)
        assert int((rl[1][b, ..., 3] > 0).sum()) > 10_000
