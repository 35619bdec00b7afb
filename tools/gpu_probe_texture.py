"""Time d3h.texture 'linear-mipmap-linear' (csrc/texture.hip) on the GPU: 1024^2 lookups into a 2048^2 x 4 texture, forward (pyramid build +
lookup) and backward (lookup backward + pyramid adjoint), with warm-up and device events.

Bytes it must move (computed from the shapes): the pyramid build reads level 0 once and writes the coarser levels (4/3 of level 0 in all);
the lookup reads uv + uv_da and writes the output (8 + 16 + 16 B per pixel) and reads the texels it touches (at most the pyramid); the
backward reads those again plus g_out, writes d_uv + d_uv_da (24 B / pixel), adds into the level gradients and gathers them back into the
base (pyramid-size read + base-size write).  Reported: times, those bytes, and bytes / time as a fraction of the HBM peak (8 TB/s).

  python tools/gpu_probe_texture.py [--iters N] [--uv coherent|random] [--out file.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'd3human-code_amd')]

import torch  # noqa: E402

HBM_PEAK = 8.0e12


def inputs(uv_kind, res=1024, size=2048, C=4):
    g = torch.Generator(device='cuda').manual_seed(0)
    tex = torch.rand(1, size, size, C, device='cuda', generator=g)
    if uv_kind == 'coherent':              # a screen-space affine map, 1.5 texels per pixel at the top of the image .. 6 at the bottom
        y, x = torch.meshgrid((torch.arange(res, device='cuda') + 0.5) / res, (torch.arange(res, device='cuda') + 0.5) / res, indexing='ij')
        s = 0.75 + 2.25 * y
        uv = torch.stack((x * s + 0.1, y * s * 0.9 + 0.05), dim=-1)[None]
        da = torch.stack((s / res, torch.zeros_like(s), torch.zeros_like(s), 0.9 * s / res), dim=-1)[None]
    else:
        uv = torch.rand(1, res, res, 2, device='cuda', generator=g)
        da = torch.randn(1, res, res, 4, device='cuda', generator=g) * 4.0 / size
    return tex, uv.contiguous(), da.contiguous()


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--uv', default='coherent', choices=('coherent', 'random'))
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'the probe needs the GPU'
    from d3h import texture as T
    tex, uv, da = inputs(a.uv)
    res, size, C = uv.shape[1], tex.shape[1], tex.shape[-1]
    npx = res * res
    sizes = T.mip_sizes(size, size)
    pyr_bytes = sum(h * w for h, w in sizes) * C * 4
    base_bytes = size * size * C * 4

    with torch.no_grad():
        t_build = timed(lambda: T.texture_construct_mip(tex), a.iters)
        pm = T.texture_construct_mip(tex)
        t_fwd_lookup = timed(lambda: T.texture(tex, uv, da, mip=pm, filter_mode='linear-mipmap-linear', boundary_mode='wrap'), a.iters)
        t_fwd = timed(lambda: T.texture(tex, uv, da, filter_mode='linear-mipmap-linear', boundary_mode='wrap'), a.iters)
    tg = tex.clone().requires_grad_(True)
    ug, dg = uv.clone().requires_grad_(True), da.clone().requires_grad_(True)
    G = torch.randn(1, res, res, C, device='cuda')

    def fwd_bwd():
        out = T.texture(tg, ug, dg, filter_mode='linear-mipmap-linear', boundary_mode='wrap')
        torch.autograd.grad(out, (tg, ug, dg), G)
    t_fb = timed(fwd_bwd, a.iters)
    t_bwd = t_fb - t_fwd

    px_fwd = npx * (8 + 16 + 16)
    bytes_fwd = pyr_bytes + px_fwd + min(pyr_bytes, npx * 8 * C * 4)          # build: base read + coarse levels written
    bytes_bwd = npx * (8 + 16 + C * 4 + 8 + 16) + 2 * min(pyr_bytes, npx * 8 * C * 4) + pyr_bytes + base_bytes
    r = {'uv': a.uv, 'lookups': f'{res}x{res}', 'texture': f'{size}x{size}x{C}', 'levels': len(sizes),
         'pyramid_build_us': round(t_build, 1), 'lookup_fwd_us': round(t_fwd_lookup, 1), 'fwd_us': round(t_fwd, 1),
         'bwd_us': round(t_bwd, 1), 'fwd_bwd_us': round(t_fb, 1),
         'fwd_bytes': bytes_fwd, 'bwd_bytes': bytes_bwd,
         'fwd_hbm_fraction': round(bytes_fwd / (t_fwd * 1e-6) / HBM_PEAK, 3), 'bwd_hbm_fraction': round(bytes_bwd / (t_bwd * 1e-6) / HBM_PEAK, 3),
         'atomic_bytes_bwd': npx * 8 * C * 4}
    print(json.dumps(r))
    if a.out:
        with open(a.out, 'a') as f:
            f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
