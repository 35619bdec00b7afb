"""Stand-alone times of what render.optixutils stands on (csrc/bvh.hip, csrc/envshade.hip, csrc/denoise.hip) on the GPU, and the resource figures
of their kernels.

    python tools/gpu_probe_optixutils.py [--out FILE.md] [--commit TEXT] [--res 1024] [--faces 100000] [--bench FILE]   # default profiles/optixutils_probe.md

 1. BVH build (d3h.raytrace.Bvh: centroid bounds, keys, torch.sort, hierarchy, refit -- the whole constructor) of a bumpy sphere of about
    --faces triangles.
 2. Bvh.occluded for res x res rays: (a) from points on the sphere along their own normals perturbed (mostly unoccluded: the ray leaves the
    surface), (b) from a point outside aimed through the mesh (every ray crosses it).
 3. env_shade forward and backward at res x res, n_samples_x = 8, 'pbr': the g-buffer is the sphere seen from outside, the shadow rays go
    against the same mesh; 128 rays per pixel and pass.
 4. bilateral_denoiser forward and backward at res x res, sigma = 2 (23 x 23 taps).
 5. VGPRs, scratch, LDS and occupancy of every kernel of the three files, from hipcc -Rpass-analysis=kernel-resource-usage where hipcc is at hand.
 6. With --bench FILE: that file's text (bench.py lines of the parent commit and of this one, taken on the same box) is copied in verbatim.

Timing: every entry is warmed up (3 calls); then REPS windows are timed with device events, each window as many back-to-back calls as make it
last about 20 ms; the table gives the per-call median and the min-max spread over the windows.  Nobody had measured any of these before: the file
records them, no test asserts them."""
import argparse
import os
import re
import statistics
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'd3human-code_amd')
for p in (os.path.join(ROOT, 'tests'), PKG):
    sys.path.insert(0, p)
import render.optixutils as ou                    # noqa: E402
from d3h import raytrace as RT, denoise as DN     # noqa: E402
from d3h import build as B                        # noqa: E402

REPS = 10


def timed(fn, reps=REPS, window_us=20000.0):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()

    def window(k):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(k):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3 / k
    k = max(1, min(200, int(window_us / max(window(1), 1.0))))
    ts = [window(k) for _ in range(reps)]
    return statistics.median(ts), min(ts), max(ts)


def fmt(t):
    return f'{t[0]:.1f} ({t[1]:.1f}-{t[2]:.1f})'


def sphere(faces, dev):
    """a unit sphere with a 5 % ripple as a lat-long grid of about `faces` triangles -> verts [V,3], tris [F,3] int32"""
    ny = max(4, int(round((faces / 4.0) ** 0.5)))
    nx = 2 * ny
    v, u = torch.meshgrid(torch.linspace(0.0, 1.0, ny + 1, device=dev), torch.arange(nx, device=dev) / nx, indexing='ij')
    theta, phi = v * np.pi, u * 2.0 * np.pi
    r = 1.0 + 0.05 * torch.sin(9.0 * theta) * torch.cos(7.0 * phi)
    verts = torch.stack([r * torch.sin(theta) * torch.cos(phi), r * torch.cos(theta), r * torch.sin(theta) * torch.sin(phi)], -1).reshape(-1, 3)
    i, j = torch.meshgrid(torch.arange(ny, device=dev), torch.arange(nx, device=dev), indexing='ij')
    a, b, c, d = i * nx + j, i * nx + (j + 1) % nx, (i + 1) * nx + j, (i + 1) * nx + (j + 1) % nx
    tris = torch.cat([torch.stack([a, c, b], -1).reshape(-1, 3), torch.stack([b, c, d], -1).reshape(-1, 3)]).int()
    return verts.float().contiguous(), tris.contiguous()


def light_tables(light):
    H, W = light.shape[:2]
    Y = ((torch.arange(H, dtype=torch.float32, device=light.device) + 0.5) / H)[:, None].expand(H, W)
    pdf = light.max(dim=-1)[0] * torch.sin(Y * np.pi)
    pdf = pdf / pdf.sum()
    cols = torch.cumsum(pdf, dim=1)
    rows = torch.cumsum(cols[:, -1:].repeat([1, W]), dim=0)
    return pdf, rows / rows[-1:, :], cols / cols[:, -1:]


def resource_rows(lines):
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    lines += ['## Kernel resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950)', '',
              'The traversal is stackless (a miss link per node), so no tracing kernel has a runtime-indexed private array: scratch is 0 everywhere.', '']
    if not os.path.exists(hipcc):
        lines += ['not collected: no hipcc on this machine', '']
        return
    lines += ['| file | kernel | VGPRs | SGPRs | scratch bytes / lane | LDS bytes / block | waves / SIMD |', '|---|---|---|---|---|---|---|']
    for f in ('bvh.hip', 'envshade.hip', 'denoise.hip'):
        cmd = [hipcc] + [x for x in B.FLAGS if x != '-shared'] + ['-Rpass-analysis=kernel-resource-usage', '-c', os.path.join(B.CSRC, f), '-o', os.devnull, '-I', B.CSRC]
        txt = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT).stdout.decode()
        demangle = lambda s: subprocess.run(['c++filt', s], stdout=subprocess.PIPE).stdout.decode().strip() if os.path.exists('/usr/bin/c++filt') else s
        for blk in txt.split('Function Name: ')[1:]:
            get = lambda k: re.search(k + r': (\d+)', blk).group(1)
            name = re.sub(r'\(anonymous namespace\)::|\(.*', '', demangle(blk.split()[0]))
            vals = [get(k) for k in ('VGPRs', 'TotalSGPRs', r'ScratchSize \[bytes/lane\]', r'LDS Size \[bytes/block\]', r'Occupancy \[waves/SIMD\]')]
            row = f'| {f} | {name} | ' + ' | '.join(vals) + ' |'
            lines.append(row)
            print(row, flush=True)
    lines.append('')


def main(dev='cuda'):
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'optixutils_probe.md'))
    ap.add_argument('--commit', default=None)
    ap.add_argument('--res', type=int, default=1024)
    ap.add_argument('--faces', type=int, default=100000)
    ap.add_argument('--bench', default=None)
    a = ap.parse_args()
    commit = a.commit
    if commit is None:
        try:
            commit = subprocess.check_output(['git', '-C', ROOT, 'rev-parse', '--short', 'HEAD'], stderr=subprocess.DEVNULL).decode().strip()
        except Exception:
            commit = 'unknown (not a git checkout)'
    res = a.res
    gen = torch.Generator().manual_seed(0)
    lines = ['# render.optixutils: BVH, occlusion query, environment shading, denoiser -- stand-alone times (tools/gpu_probe_optixutils.py)', '',
             f'Commit: {commit}.  Device: {torch.cuda.get_device_name(0)}.  One run of the probe; {REPS} timed windows of about 20 ms per entry; us per call: '
             'median (min-max).', 'Nothing here is a gate: the tests assert occlusion exactly and parity of the float outputs, no time.', '']
    verts, tris = sphere(a.faces, dev)
    F = int(tris.shape[0])
    rows = [('BVH build (Bvh constructor, sort included)', f'F = {F}, V = {verts.shape[0]}', timed(lambda: RT.Bvh(verts, tris)))]
    bvh = RT.Bvh(verts, tris)
    # g-buffer: the sphere seen from outside; pixel (y, x) looks at the point of direction (theta, phi)
    vv, uu = torch.meshgrid((torch.arange(res, device=dev) + 0.5) / res, (torch.arange(res, device=dev) + 0.5) / res, indexing='ij')
    theta, phi = vv * np.pi, uu * 2.0 * np.pi
    nrm = torch.stack([torch.sin(theta) * torch.cos(phi), torch.cos(theta), torch.sin(theta) * torch.sin(phi)], -1)[None].float().contiguous()
    pos = nrm * (1.0 + 0.05 * torch.sin(9.0 * theta) * torch.cos(7.0 * phi))[None, ..., None]
    ro = (pos + 0.01 * nrm).contiguous()
    d_out = torch.nn.functional.normalize(nrm + 0.7 * torch.randn(1, res, res, 3, generator=gen).to(dev), dim=-1)
    eye = torch.tensor([0.0, 0.0, 4.0], device=dev).expand(1, res, res, 3).contiguous()
    d_in = (pos - eye).contiguous()
    with torch.no_grad():
        share = lambda o, d: f'{float(bvh.occluded(o, d).float().mean()):.2f} of the rays occluded'
        rows.append((f'occluded, {res}^2 rays leaving the surface', f'F = {F}; {share(ro, d_out)}', timed(lambda: bvh.occluded(ro, d_out))))
        rows.append((f'occluded, {res}^2 rays through the mesh', f'F = {F}; {share(eye, d_in)}', timed(lambda: bvh.occluded(eye, d_in))))
    # environment shading
    light = (torch.rand(256, 512, 3, generator=gen) * 3.9 + 0.1).to(dev)
    pdf, lrows, cols = light_tables(light)
    kd = torch.rand(1, res, res, 3, generator=gen).to(dev) * 0.8 + 0.1
    ks = torch.stack([torch.rand(res, res, generator=gen) * 0.5, torch.rand(res, res, generator=gen) * 0.6 + 0.3, torch.rand(res, res, generator=gen)], -1)[None].to(dev)
    mask = torch.ones(1, res, res, device=dev)
    ctx = ou.OptiXContext()
    ou.optix_build_bvh(ctx, verts, tris, rebuild=1)
    leaves = [t.detach().requires_grad_(True) for t in (pos, nrm, kd, ks, light)]

    def shade():
        return ou.optix_env_shade(ctx, mask, ro, leaves[0], leaves[1], eye, leaves[2], leaves[3], leaves[4], pdf, lrows[:, 0], cols, BSDF='pbr', n_samples_x=8,
                                  rnd_seed=7)
    with torch.no_grad():
        rows.append((f"optix_env_shade forward, {res}^2, n_samples_x = 8, 'pbr'", f'F = {F}, light 256 x 512; 128 shadow rays per pixel', timed(shade)))
    diff, spec = shade()
    g = torch.randn_like(diff)
    rows.append((f"optix_env_shade backward, {res}^2, n_samples_x = 8, 'pbr'", 'gradients of gb_pos, gb_normal, gb_kd, gb_ks, light; re-traces the 128 rays',
                 timed(lambda: torch.autograd.grad([diff, spec], leaves, [g, g], retain_graph=True))))
    del diff, spec
    # denoiser
    col = torch.rand(1, res, res, 3, generator=gen).to(dev)
    zdz = torch.stack([2.0 + 0.2 * torch.rand(res, res, generator=gen), torch.rand(res, res, generator=gen) * 0.99 + 0.01], -1)[None].to(dev)
    with torch.no_grad():
        rows.append((f'bilateral_denoiser forward, {res}^2, sigma 2', '23 x 23 taps per pixel, staged through LDS', timed(lambda: DN.bilateral_denoise(col, nrm, zdz, 2.0))))
    leaf = col.detach().requires_grad_(True)
    out = DN.bilateral_denoise(leaf, nrm, zdz, 2.0)
    g4 = torch.randn_like(out)
    rows.append((f'bilateral_denoiser backward, {res}^2, sigma 2', 'd col, a gather', timed(lambda: torch.autograd.grad(out, [leaf], g4, retain_graph=True))))
    lines += ['## Times', '', '| what | setting | us per call |', '|---|---|---|']
    for what, setting, t in rows:
        row = f'| {what} | {setting} | {fmt(t)} |'
        lines.append(row)
        print(row, flush=True)
    lines.append('')
    resource_rows(lines)
    if a.bench:
        lines += ['## bench.py before and after (same box, same call)', '',
                  'optix_build_bvh stores two references and launches nothing, so the training step does not change; the lines below are the plain bench.py '
                  'result lines of the parent commit and of this one, run alternately.', '', '```'] + open(a.bench).read().splitlines() + ['```', '']
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, 'w').write('\n'.join(lines) + '\n')
    print(f'wrote {a.out}')


if __name__ == '__main__':
    assert torch.cuda.is_available(), 'needs the GPU'
    main()
