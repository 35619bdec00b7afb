"""Time the pixel-derivative gradients of csrc/raster.hip on the GPU at 4 x 1024^2, with warm-up and device events: rasterize backward with
and without g_db, interpolate backward with and without g_da (a 2-channel uv attribute, diff_attrs='all'), for a ~10 k and a ~100 k random
triangle mesh; and the end-to-end rasterize -> interpolate -> texture('linear-mipmap-linear') backward of a receding quad into a 2048^2 x 4
texture.

Bytes each backward must move (computed from the shapes): rasterize reads rast + g_rast (+ g_db) per pixel (32 or 48 B) and writes d_pos;
interpolate reads rast + g_out (+ db + g_da) and writes d_rast (+ d_rast_db) per pixel (16 + 4A + 16, + 16 + 8A + 16) plus the attribute
atomics.  Reported: times, those bytes, and bytes / time as a fraction of the HBM peak (8 TB/s).

  python tools/gpu_probe_raster_db.py [--iters N] [--out file.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'd3human-code_amd')]

import torch  # noqa: E402

HBM_PEAK = 8.0e12


def timed(fn, iters):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters          # us


def random_mesh(nf, B, size, seed=0):
    g = torch.Generator(device='cuda').manual_seed(seed)
    cen = (torch.rand(B, nf, 1, 2, device='cuda', generator=g) * 2 - 1) * 0.9
    xy = (cen + (torch.rand(B, nf, 3, 2, device='cuda', generator=g) * 2 - 1) * size).reshape(B, nf * 3, 2)
    z = torch.rand(B, nf * 3, 1, device='cuda', generator=g) * 1.6 - 0.8
    w = torch.rand(B, nf * 3, 1, device='cuda', generator=g) * 2 + 1
    return torch.cat([xy * w, z * w, w], -1).contiguous(), torch.arange(nf * 3, dtype=torch.int32, device='cuda').reshape(nf, 3)


def probe_mesh(nf, size, B, res, iters):
    from d3h import raster
    pos, tri = random_mesh(nf, B, size)
    npx = B * res * res
    p = pos.clone().requires_grad_(True)
    rast, db = raster.rasterize(p, tri, (res, res), grad_db=True)
    g_rast, g_db = torch.randn_like(rast), torch.randn_like(db)
    t_r = timed(lambda: torch.autograd.grad(rast, p, g_rast, retain_graph=True), iters)
    t_rdb = timed(lambda: torch.autograd.grad((rast, db), p, (g_rast, g_db), retain_graph=True), iters)
    A = 2
    attr = torch.rand(1, pos.shape[1], A, device='cuda').requires_grad_(True)
    r_ = rast.detach().requires_grad_(True)
    d_ = db.detach().requires_grad_(True)
    out, da = raster.interpolate(attr, r_, tri, rast_db=d_, diff_attrs='all')
    g_out, g_da = torch.randn_like(out), torch.randn_like(da)
    t_i = timed(lambda: torch.autograd.grad(out, (attr, r_), g_out, retain_graph=True), iters)
    t_ida = timed(lambda: torch.autograd.grad((out, da), (attr, r_, d_), (g_out, g_da), retain_graph=True), iters)
    cov = float((rast[..., 3] > 0).float().mean())
    b_r, b_rdb = npx * 32, npx * 48
    b_i, b_ida = npx * (16 + 4 * A + 16), npx * (16 + 4 * A + 16 + 16 + 8 * A + 16)
    f = lambda b, t: round(b / (t * 1e-6) / HBM_PEAK, 3)
    return {'mesh': f'{nf // 1000}k random', 'frames': f'{B}x{res}^2', 'covered': round(cov, 3),
            'raster_bwd_us': round(t_r, 1), 'raster_bwd_db_us': round(t_rdb, 1),
            'raster_bwd_hbm': f(b_r, t_r), 'raster_bwd_db_hbm': f(b_rdb, t_rdb),
            'interp_bwd_us': round(t_i, 1), 'interp_bwd_da_us': round(t_ida, 1),
            'interp_bwd_hbm': f(b_i, t_i), 'interp_bwd_da_hbm': f(b_ida, t_ida)}


def probe_chain(B, res, size, iters):
    import nvdiffrast.torch as dr
    wf = 400.0
    pos = torch.tensor([[-0.9, -0.9, 0.5, 1.0], [0.9, -0.9, 0.5, 1.0], [-0.9 * wf, 0.99 * wf, 0.9 * wf, wf], [0.9 * wf, 0.99 * wf, 0.9 * wf, wf]],
                       device='cuda')[None].expand(B, -1, -1).contiguous()
    tri = torch.tensor([[0, 1, 2], [2, 1, 3]], dtype=torch.int32, device='cuda')
    uv_attr = torch.tensor([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0], [1.0, 1.0]], device='cuda')
    tex = torch.rand(1, size, size, 4, device='cuda')
    p, ua, tk = pos.requires_grad_(True), uv_attr.requires_grad_(True), tex.requires_grad_(True)

    def fwd(grad_db):
        rast, db = dr.rasterize(None, p, tri, (res, res), grad_db=grad_db)
        uv, uv_da = dr.interpolate(ua, rast, tri, rast_db=db, diff_attrs='all')
        return dr.texture(tk, uv, uv_da, filter_mode='linear-mipmap-linear', boundary_mode='wrap')
    G = torch.randn(B, res, res, 4, device='cuda')
    with torch.no_grad():
        t_f = timed(lambda: fwd(True), iters)
    t_fb = timed(lambda: torch.autograd.grad(fwd(True), (p, ua, tk), G), iters)
    t_fb0 = timed(lambda: torch.autograd.grad(fwd(False), (p, ua, tk), G), iters)
    return {'chain': f'receding quad {B}x{res}^2, texture {size}^2x4 linear-mipmap-linear', 'fwd_us': round(t_f, 1),
            'bwd_us': round(t_fb - t_f, 1), 'bwd_us_grad_db_false': round(t_fb0 - t_f, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'the probe needs the GPU'
    rows = [probe_mesh(10_000, 0.04, 4, 1024, a.iters), probe_mesh(100_000, 0.012, 4, 1024, a.iters), probe_chain(4, 1024, 2048, a.iters)]
    for r in rows:
        print(json.dumps(r))
        if a.out:
            with open(a.out, 'a') as f:
                f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
