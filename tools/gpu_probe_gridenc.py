"""Stand-alone times of the general grid encoding (csrc/gridenc.hip) on the GPU: forward, table-gradient half and position-gradient half.

    python tools/gpu_probe_gridenc.py [--points N] [--out FILE.md]          # defaults 4 x 1024^2, profiles/gridenc_probe.md

 1. the general kernels on the REFERENCE configuration beside the fused kernels' own encoding (d3h_texmlp_fwd / d3h_texmlp_bwd in their
    encoding-only mode: the code the product runs for that configuration), same inputs: what generality costs;
 2. the 16-level grid at log2_hashmap_size 19 and 21 beside (a) a float32 torch restatement on the same GPU (gather, `index_add_`), which is
    what the shim would otherwise call, and (b) the atomic-rate floors of DESIGN.md section 3: N x hashed levels x 2^D corners x 4 F bytes
    at 0.08 TB/s (one lane per row) and at 1.3 TB/s (contiguous adds).
Points: uniformly random, and pixel-coherent -- the position buffer of the synthetic scene's body (an ellipsoid seen along z, one position per
pixel, background pixels at the origin), normalised and clamped by the texture's box exactly as MLPTexture3D.sample does.

Timing: every entry is warmed up (3 launches), then REPS launches are timed one by one with device events; the table reports the median and
the min-max spread.  Tables (4-180 MB) and point sets (50-540 MB per buffer) are larger than the 32 MiB of L2; the Infinity Cache (256 MiB)
does hold a level's slice between launches, which is the design's premise, not an artefact."""
import argparse
import ctypes
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'd3human-code_amd'))
from d3h import _lib as L, gridenc, texmlp        # noqa: E402

REPS = 10
PLS = texmlp.PER_LEVEL_SCALE
BBOX = (0.6, 0.6, 0.2, -0.8, -1.2, -0.2)


def timed(fn, reps=REPS):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return statistics.median(ts), min(ts), max(ts)          # us


def fmt(t):
    return f'{t[0]:9.1f} ({t[1]:.1f}-{t[2]:.1f})'


def random_points(n, dev):
    return torch.rand(n, 3, generator=torch.Generator().manual_seed(0)).to(dev)


def coherent_points(n, dev):
    """frames of res x res pixels looking along z at the ellipsoid of the synthetic scene (centre (0, -0.4, 0), radii (0.55, 0.8, 0.45)):
    the front surface point per covered pixel, the origin elsewhere; then the box normalisation + clamp of MLPTexture3D.sample"""
    res = int(round(math.sqrt(n / 4)))
    frames = max(1, n // (res * res))
    u = (torch.arange(res, device=dev, dtype=torch.float32) + 0.5) / res * 2 - 1
    py, px = torch.meshgrid(u * 1.3 - 0.4, u * 1.3, indexing='ij')
    out = []
    for f in range(frames):
        ox = px + 0.01 * f
        r2 = (ox / 0.55) ** 2 + ((py + 0.4) / 0.8) ** 2
        z = 0.45 * torch.sqrt(torch.clamp(1 - r2, min=0))
        pos = torch.stack([ox, py, z], -1) * (r2 < 1)[..., None]
        out.append(pos.reshape(-1, 3))
    x = torch.cat(out)[:n]
    b0, b1 = torch.tensor(BBOX[:3], device=dev), torch.tensor(BBOX[3:], device=dev)
    return torch.clamp((x - b0) / (b1 - b0), 0, 1).contiguous()


def torch_levels(x, cfg):
    """per level: (entry index [2^D][N] int64 into the whole table, corner weight [2^D][N]) in float32 torch ops"""
    for l in range(cfg.n_levels):
        p = torch.addcmul(torch.full_like(x, 0.5), x, torch.full_like(x, cfg.scale[l]))
        fl = torch.floor(p)
        fr = p - fl
        q = fl.long()
        idx, w = [], []
        for c in range(8):
            wc, qs = 1.0, []
            for d in range(3):
                bit = (c >> d) & 1
                wc = wc * (fr[:, d] if bit else 1 - fr[:, d])
                qs.append(q[:, d] + bit)
            if cfg.hashed[l]:
                i = qs[0] ^ ((qs[1] * 2654435761) & 0xFFFFFFFF) ^ ((qs[2] * 805459861) & 0xFFFFFFFF)
            else:
                i = qs[0] + qs[1] * cfg.res[l] + qs[2] * cfg.res[l] ** 2
            idx.append(i % cfg.size[l] + cfg.offset[l])
            w.append(wc)
        yield l, idx, w


def torch_fwd(x, tab2, cfg):
    return torch.cat([sum(w[c][:, None] * tab2[idx[c]] for c in range(8)) for _, idx, w in torch_levels(x, cfg)], -1)


def torch_bwd_table(x, tab2, g, cfg):
    dt = torch.zeros_like(tab2)
    F = cfg.n_features
    for l, idx, w in torch_levels(x, cfg):
        for c in range(8):
            dt.index_add_(0, idx[c], w[c][:, None] * g[:, l * F:(l + 1) * F])
    return dt


def probe(cfg, x, label, lines, with_torch, with_fused):
    dev = x.device
    n = x.shape[0]
    lib = L.lib()
    F = cfg.n_features
    tab = ((torch.rand(cfg.n_params, generator=torch.Generator().manual_seed(1)) - 0.5)).to(dev)
    g = torch.randn(n, cfg.n_output_dims, generator=torch.Generator().manual_seed(2)).to(dev)
    out = torch.empty(n, cfg.n_output_dims, device=dev)
    d_tab, d_x = torch.zeros_like(tab), torch.zeros_like(x)
    ka = cfg._kernel_args()
    nf = L.i64(tab.numel())
    run = lambda rc: L.check(rc, 'probe')
    t_f = timed(lambda: run(lib.d3h_gridenc_fwd(L.ptr(x), L.ptr(tab), nf, L.i64(n), *ka, L.ptr(out), L.stream())))
    t_t = timed(lambda: run(lib.d3h_gridenc_bwd(L.ptr(x), L.ptr(tab), nf, L.ptr(g), L.i64(n), *ka, L.ptr(d_tab), None, L.stream())))
    t_x = timed(lambda: run(lib.d3h_gridenc_bwd(L.ptr(x), L.ptr(tab), nf, L.ptr(g), L.i64(n), *ka, None, L.ptr(d_x), L.stream())))
    nh = sum(cfg.hashed)
    bytes_h = n * nh * 8 * 4 * F
    row = f'| {label} | general (csrc/gridenc.hip) | {fmt(t_f)} | {fmt(t_t)} | {fmt(t_x)} |'
    lines.append(row)
    print(row, flush=True)
    if nh:
        row = (f'| {label} | floor: {nh} hashed levels, {bytes_h / 1e9:.2f} GB of scattered adds |  | {bytes_h / 0.08e12 * 1e6:.0f} at 0.08 TB/s; '
               f'{bytes_h / 1.3e12 * 1e6:.0f} at 1.3 TB/s |  |')
        lines.append(row)
        print(row, flush=True)
    if with_fused:
        unit = (ctypes.c_float * 6)(0, 0, 0, 1, 1, 1)
        pa = (ctypes.c_double(PLS), L.i32(16), unit)
        f_f = timed(lambda: run(lib.d3h_texmlp_fwd(L.ptr(x), None, L.ptr(tab), None, L.i64(n), *pa, None, None, None, L.ptr(out), L.stream())))
        bw = lambda dt, dx: run(lib.d3h_texmlp_bwd(L.ptr(x), None, L.ptr(tab), None, L.i64(n), *pa, None, None, L.f32(1.0), L.i32(1), L.ptr(g),
                                                   L.ptr(dt), None, L.ptr(dx), None, L.stream()))
        f_t = timed(lambda: bw(d_tab, None))
        f_x = timed(lambda: bw(None, d_x))
        row = f'| {label} | fused kernels, encoding only (csrc/texmlp.hip) | {fmt(f_f)} | {fmt(f_t)} | {fmt(f_x)} |'
        lines.append(row)
        print(row, flush=True)
        row = f'| {label} | ratio general / fused | {t_f[0] / f_f[0]:.2f} | {t_t[0] / f_t[0]:.2f} | {t_x[0] / f_x[0]:.2f} |'
        lines.append(row)
        print(row, flush=True)
    if with_torch:
        tab2 = tab.view(-1, F)
        with torch.no_grad():
            o_f = timed(lambda: torch_fwd(x, tab2, cfg), reps=3)
            o_t = timed(lambda: torch_bwd_table(x, tab2, g, cfg), reps=3)

        def dx_torch():
            xr = x.detach().requires_grad_(True)
            (torch_fwd(xr, tab2, cfg) * g).sum().backward()
        o_x = timed(dx_torch, reps=3)
        row = f'| {label} | torch float32 restatement (gather / index_add_ / autograd for x, forward included) | {fmt(o_f)} | {fmt(o_t)} | {fmt(o_x)} |'
        lines.append(row)
        print(row, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--points', type=int, default=4 * 1024 * 1024)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'gridenc_probe.md'))
    a = ap.parse_args()
    dev = 'cuda'
    n = a.points
    lines = ['# General grid encoding: stand-alone kernel times (tools/gpu_probe_gridenc.py)', '',
             f'{n} points, 3-D, 2 features per entry; us per launch, median of {REPS} single launches timed with device events (min-max); the torch',
             'rows: 3 launches.  "table grad" and "position grad" are the two halves of the backward, each launched alone.', '',
             '| configuration, points | code | forward | table grad | position grad |', '|---|---|---|---|---|']
    ref = {'otype': 'Grid', 'type': 'Hash', 'n_levels': 5, 'n_features_per_level': 2, 'log2_hashmap_size': 21, 'base_resolution': 16, 'per_level_scale': PLS}
    pts = {'random': random_points(n, dev), 'pixel-coherent': coherent_points(n, dev)}
    for name, x in pts.items():
        probe(gridenc.GridConfig(3, ref), x, f'reference (5 dense levels), {name}', lines, with_torch=False, with_fused=True)
    for T in (19, 21):
        c = dict(ref, n_levels=16, log2_hashmap_size=T)
        for name, x in pts.items():
            probe(gridenc.GridConfig(3, c), x, f'16 levels T={T}, {name}', lines, with_torch=True, with_fused=False)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, 'w').write('\n'.join(lines) + '\n')
    print(f'wrote {a.out}')


if __name__ == '__main__':
    assert torch.cuda.is_available(), 'needs the GPU'
    main()
