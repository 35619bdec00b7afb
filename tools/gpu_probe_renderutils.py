"""Stand-alone times and error ratios of the BSDF and cube-map entry points of render.renderutils (csrc/bsdf.hip, csrc/cubemap.hip) on the GPU.

    python tools/gpu_probe_renderutils.py [--out FILE.md] [--commit TEXT] [--res 1024] [--spec-n 128]     # default profiles/renderutils_probe.md

 1. pbr_bsdf (both diffuse lobes) and pbr_specular at res x res, B = 1, view_pos / light_pos broadcast [1,1,1,3]: forward, and backward (a) with
    every input requiring a gradient and (b) with the material inputs only (kd, arm / col, alpha) -- beside the package's own torch
    composition (`use_python=True`) on the same inputs.  Backward = torch.autograd.grad on a retained graph: the kernel plus the wrapper's
    sums of the broadcast inputs' gradients, nothing of the forward.
 2. diffuse_cubemap at N = 16 and specular_cubemap at N = --spec-n with roughness 0.08, 0.3, 0.5: forward and backward beside a dense torch
    matmul with the precomputed weight matrix [6 N^2, 6 N^2] (building the matrix is not timed; at N = 128 it is 38.7 GB and is only built when
    that much device memory is free twice over -- otherwise the row says "not measured").
 3. the parity figures of tests/renderutils_cases.py on this GPU: max|got - f64| / max|f64| over the bound max(5 ref32_err, 2^-20), per case.

Timing: every entry is warmed up (3 calls); then REPS windows are timed with device events, each window as many back-to-back calls as make it
last about 2 ms; the table gives the per-call median and the min-max spread over the windows, in us.  No speed-up is gated anywhere: the file
records what was measured, and says so where a kernel loses."""
import argparse
import contextlib
import io
import os
import statistics
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'd3human-code_amd')):
    sys.path.insert(0, p)
import render.renderutils as ru                  # noqa: E402
from d3h import cubemap as DC                    # noqa: E402

REPS = 10


def timed(fn, reps=REPS, window_us=2000.0):
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
    return 'not measured' if t is None else f'{t[0]:.1f} ({t[1]:.1f}-{t[2]:.1f})'


def ratio(a, b):
    """torch time over HIP time; below 1 the HIP kernel loses, and the row says so"""
    if a is None or b is None:
        return ''
    r = a[0] / b[0]
    return f'{r:.2f}' + (' (the HIP kernel loses)' if r < 1.0 else '')


def unit(*shape, gen, dev):
    return torch.nn.functional.normalize(torch.randn(*shape, generator=gen), dim=-1).to(dev)


def bsdf_rows(res, dev, lines):
    gen = torch.Generator().manual_seed(0)
    u = lambda *s: torch.rand(*s, generator=gen).to(dev)
    full = (1, res, res)
    pos = u(*full, 3) - 0.5
    view_pos = torch.tensor([0.3, -0.2, 3.0], device=dev).view(1, 1, 1, 3)
    light_pos = torch.tensor([-0.5, 2.5, 1.0], device=dev).view(1, 1, 1, 3)
    nrm = torch.nn.functional.normalize(0.6 * torch.nn.functional.normalize(light_pos - pos, dim=-1) + unit(*full, 3, gen=gen, dev=dev), dim=-1)
    pbr = dict(kd=u(*full, 3), arm=u(*full, 3), pos=pos, nrm=nrm, view_pos=view_pos, light_pos=light_pos)
    spec = dict(col=u(*full, 3), nrm=nrm, wo=torch.nn.functional.normalize(view_pos - pos, dim=-1), wi=torch.nn.functional.normalize(light_pos - pos, dim=-1),
                alpha=u(*full, 1))
    ops = [('pbr_bsdf, lambert', pbr, ('kd', 'arm'), lambda py, *a: ru.pbr_bsdf(*a, use_python=py)),
           ('pbr_bsdf, frostbite', pbr, ('kd', 'arm'), lambda py, *a: ru.pbr_bsdf(*a, bsdf='frostbite', use_python=py)),
           ('pbr_specular', spec, ('col', 'alpha'), lambda py, *a: ru.pbr_specular(*a, use_python=py))]
    lines += [f'## Per-pixel BSDF functions at {res} x {res}, B = 1, view_pos / light_pos [1,1,1,3]', '',
              'us per call: median (min-max).  "all": every input requires a gradient; "material": only the named ones do.', '',
              '| function | code | forward | backward, all | backward, material | ', '|---|---|---|---|---|']
    for name, ins, material, fn in ops:
        res_t = {}
        for py in (False, True):
            vals = [v.detach() for v in ins.values()]
            with torch.no_grad():
                t_f = timed(lambda: fn(py, *vals))
            t_b = []
            for want in (tuple(ins), material):
                leaves = [v.detach().requires_grad_(k in want) for k, v in ins.items()]
                out = fn(py, *leaves)
                g = torch.randn_like(out)
                need = [l for l in leaves if l.requires_grad]
                t_b.append(timed(lambda: torch.autograd.grad(out, need, g, retain_graph=True)))
                del out
            res_t[py] = (t_f, *t_b)
            code = 'torch composition (use_python=True)' if py else 'HIP kernels (csrc/bsdf.hip)'
            row = f'| {name} | {code} | {fmt(t_f)} | {fmt(t_b[0])} | {fmt(t_b[1])} ({", ".join(material)}) |'
            lines.append(row)
            print(row, flush=True)
        row = f'| {name} | ratio torch / HIP | ' + ' | '.join(ratio(res_t[True][k], res_t[False][k]) for k in range(3)) + ' |'
        lines.append(row)
        print(row, flush=True)
    lines.append('')


def weight_rows(table, rows, roughness, cut):
    """rows [r0, r1) of the diffuse / specular weight matrices from the texel table, in float32 torch ops"""
    d, area = table[:, :3], table[:, 3]
    dp = d[rows[0]:rows[1]]
    dots = dp @ d.T
    if roughness is None:
        return dots.clamp(0.0, 0.999) * area[None, :] / 3.141592
    h = torch.nn.functional.normalize(dp[:, None, :] + d[None, :, :], dim=-1)
    c = (dp[:, None, :] * h).sum(-1).clamp(0.0, 1.0)
    a2 = float(roughness) ** 4
    dd = (c * a2 - c) * c + 1.0
    return torch.where(dots >= cut, dots.clamp(min=0.0) * (a2 / (dd * dd * np.pi)) * area[None, :] / 4.0, torch.zeros_like(dots))


def dense_weights(N, roughness, dev):
    n = 6 * N * N
    free, _ = torch.cuda.mem_get_info()
    if 2 * 4 * n * n + (4 << 30) > free:
        return None
    table = DC.texel_table(N, dev)[0]
    cut = None if roughness is None else DC.costheta_cutoff(N, roughness, 0.99)
    Wm = torch.empty(n, n, device=dev)
    step = max(1, min(n, (1 << 26) // n))
    for r0 in range(0, n, step):
        Wm[r0:r0 + step] = weight_rows(table, (r0, min(n, r0 + step)), roughness, cut)
    return Wm


def cubemap_rows(spec_n, dev, lines):
    lines += ['## Cube-map filters', '',
              'us per call: median (min-max).  "dense torch matmul": W @ c and W^T @ g with the precomputed [6 N^2, 6 N^2] weight matrix (for the '
              'specular filter W is normalised by its row sums beforehand, so both sides do the same work per call).', '',
              'The kernels sweep texel pairs in 16 x 16 patches and skip the patches the filter cannot reach, so their time follows the cone: a narrow '
              'lobe touches a few patches, roughness 0.5 (cutoff angle 63 degrees) about half the cube, the diffuse filter a hemisphere.  The dense '
              'matmul does the same work whatever the lobe, but needs the weight matrix: 38.7 GB at N = 128, built by torch ops that are not timed here.',
              'At N = 16 the whole cube is six workgroups; the sweep is a chain of 1536 dependent steps per thread on six compute units.',
              '"against float64": at N = 128 some texel pairs lie within float32 rounding of the cutoff, and a pair that falls on the other side '
              'moves that output texel by a few per cent (on the host, a float32 numpy evaluation of 256 texels at roughness 0.08 had 1 such pair in '
              '3327 and was 2.2e-2 off on that texel); the torch float32 matrix shows the same.  It is a property of the hard cutoff in float32, in the '
              'reference\'s kernels as well; the tests use sizes where no pair is that close.', '',
              '| filter | code | forward | backward |', '|---|---|---|---|']
    for name, N, roughness in [('diffuse_cubemap, N = 16', 16, None)] + [(f'specular_cubemap, N = {spec_n}, roughness {r}', spec_n, r) for r in (0.08, 0.3, 0.5)]:
        gen = torch.Generator().manual_seed(N)
        c = (torch.rand(6, N, N, 3, generator=gen) * 4.0).to(dev)
        g = torch.randn(6, N, N, 3, generator=gen).to(dev)
        fn = (lambda x: ru.diffuse_cubemap(x)) if roughness is None else (lambda x: ru.specular_cubemap(x, roughness))
        with torch.no_grad():
            t_f = timed(lambda: fn(c))
        leaf = c.detach().requires_grad_(True)
        out = fn(leaf)
        t_b = timed(lambda: torch.autograd.grad(out, [leaf], g, retain_graph=True))
        row = f'| {name} | HIP kernels (csrc/cubemap.hip) | {fmt(t_f)} | {fmt(t_b)} |'
        lines.append(row)
        print(row, flush=True)
        if roughness is not None:
            # accuracy at this size: 512 output texels against the same formulas in float64 torch ops (the full brute-force yardstick of the
            # tests does not fit at N = 128)
            tab64 = DC.texel_table(N, dev)[0].double()
            rows = torch.randperm(6 * N * N, generator=gen)[:512].to(dev)
            W64 = torch.cat([weight_rows(tab64, (int(r), int(r) + 1), roughness, DC.costheta_cutoff(N, roughness, 0.99)) for r in rows])
            ref = (W64 @ c.reshape(-1, 3).double()) / W64.sum(1, keepdim=True)
            e64 = ((out.detach().reshape(-1, 3)[rows] - ref).abs().max() / ref.abs().max()).item()
            row = f'| {name} | forward of the HIP kernels against float64 on 512 random texels: {e64:.1e} of the largest element | | |'
            lines.append(row)
            print(row, flush=True)
            del W64, tab64
        Wm = dense_weights(N, roughness, dev)
        m_f = m_b = None
        if Wm is not None:
            if roughness is not None:
                Wm /= Wm.sum(1, keepdim=True)
            cf, gf = c.reshape(-1, 3), g.reshape(-1, 3)
            err = ((Wm @ cf) - out.detach().reshape(-1, 3)).abs().max().item() / out.detach().abs().max().item()
            m_f = timed(lambda: Wm @ cf)
            m_b = timed(lambda: Wm.T @ gf)
            note = f'; its forward differs from the kernels\' by {err:.1e} of the largest element'
        else:
            note = f': the {4 * (6 * N * N) ** 2 / 1e9:.1f} GB matrix does not fit twice into the free device memory'
        row = f'| {name} | dense torch matmul{note} | {fmt(m_f)} | {fmt(m_b)} |'
        lines.append(row)
        print(row, flush=True)
        row = f'| {name} | ratio torch / HIP | {ratio(m_f, t_f)} | {ratio(m_b, t_b)} |'
        lines.append(row)
        print(row, flush=True)
        del Wm, out
        torch.cuda.empty_cache()
    lines.append('')


def parity_rows(dev, lines):
    """the figures the tests assert, as tests/renderutils_cases.py prints them: error, bound, and their ratio"""
    import renderutils_cases as RC
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        for case in RC.CASES:
            RC.check_parity(dev, case)
        for N in RC.CUBE_NS:
            for r in RC.CUBE_ROUGHNESS:
                RC.check_cubemap(dev, N, r)
    figures = [l for l in buf.getvalue().splitlines() if 'of it)' in l]
    worst = max(float(l.split(',')[-1].split('of it')[0]) for l in figures)
    lines += ['## Parity on this GPU', '',
              'max|got - f64| / max|f64| per tensor against the float64 yardstick, the bound max(5 ref32_err, 2^-20), and the share of the bound used '
              '(tests/renderutils_cases.py: the reference\'s python twins for the per-pixel functions, the sum over all texel pairs for the cube maps).',
              f'Largest share of a bound: {worst:.2f}.', '', '```'] + figures + ['```', '']
    print(f'parity: largest share of a bound {worst:.2f}', flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'renderutils_probe.md'))
    ap.add_argument('--commit', default=None)
    ap.add_argument('--res', type=int, default=1024)
    ap.add_argument('--spec-n', type=int, default=128)
    a = ap.parse_args()
    commit = a.commit
    if commit is None:
        try:
            commit = subprocess.check_output(['git', '-C', ROOT, 'rev-parse', '--short', 'HEAD'], stderr=subprocess.DEVNULL).decode().strip()
        except Exception:
            commit = 'unknown (not a git checkout)'
    dev = 'cuda'
    lines = ['# render.renderutils BSDF and cube-map entry points: stand-alone times and parity (tools/gpu_probe_renderutils.py)', '',
             f'Commit: {commit}.  Device: {torch.cuda.get_device_name(0)}.  One run of the probe; {REPS} timed windows of about 2 ms per entry.',
             'Nothing here is a gate: the tests assert parity only.', '']
    bsdf_rows(a.res, dev, lines)
    cubemap_rows(a.spec_n, dev, lines)
    parity_rows(dev, lines)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, 'w').write('\n'.join(lines) + '\n')
    print(f'wrote {a.out}')


if __name__ == '__main__':
    assert torch.cuda.is_available(), 'needs the GPU'
    main()
