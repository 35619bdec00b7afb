"""Times of the lit render path on the GPU: the light's tables, the two-image denoiser, and one lit tick_init step beside the unlit one.

    python tools/gpu_probe_lit.py [--out FILE.md] [--commit TEXT] [--res 1024] [--grid 63] [--frames 4] [--no-trace]      # default profiles/lit_probe.md

 1. EnvironmentLight.update_pdf at 256 x 256: the kernel pair of csrc/envlight.hip (d3h.envlight.tables) against the torch composition of
    render/light.py:46-59 (about ten launches), alternating; the largest difference between the two results.
 2. The denoiser under one set of guides: d3h.denoise.bilateral_denoise_many([a, b]) against two bilateral_denoise calls, 512^2 and 1024^2, sigma 2
    (23 x 23 taps), forward and backward, alternating; the results are compared bit for bit first.
 3. One tick_init step (forward, backward, optimiser step) of the synthetic scene at the benchmark's config-3 shape (--grid 63: tet resolution 128; --res 1024,
    --frames 4, full loss stack): FLAGS.lit_shading with bsdf 'pbr', n_samples 4 and the bilateral denoiser, beside the same step with the flag off
    -- the 'kd' path, whose code the flag does not touch -- alternating; then, unless --no-trace, each step once more in a child process under
    `rocprofv3 --kernel-trace --stats` for the per-kernel split of the steps that follow a marker dispatch (tracing slows the host: the end-to-end
    times come from the untraced run).

Timing: every entry is warmed up (3 calls); then REPS windows are timed with device events, each window as many back-to-back calls as make it last
about 20 ms (steps: one step per window); the tables give the per-call median and the min-max spread.  Two variants of one entry are timed
alternately, window by window.  No test asserts any of these numbers; `shade_lit` keeps `forward_many` only while section 2 shows it no slower than
two single calls -- the file's verdict line says which way that went."""
import argparse
import csv
import glob
import os
import statistics
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'd3human-code_amd')
for p in (os.path.join(ROOT, 'tests'), PKG):
    sys.path.insert(0, p)
from d3h import denoise as DN, envlight as EL          # noqa: E402

REPS = 10
MARK_ROWS = 7            # the light map of the trace marker: an envlight_row_kernel launch of 7 workgroups, a grid no step launches


def _window(fn, k):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(k):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / k


def timed_pair(fns, reps=REPS, window_us=20000.0, k=None):
    """-> one (median, min, max) in us per call for each of `fns`, their windows alternating"""
    for fn in fns:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ks = [k or max(1, min(200, int(window_us / max(_window(fn, 1), 1.0)))) for fn in fns]
    ts = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            ts[i].append(_window(fn, ks[i]))
    return [(statistics.median(t), min(t), max(t)) for t in ts]


def fmt(t):
    return f'{t[0]:.1f} ({t[1]:.1f}-{t[2]:.1f})'


def torch_tables(base):
    """render/light.py:46-59 as a torch composition (what update_pdf replaces)"""
    H, W = base.shape[:2]
    Y = ((torch.arange(H, dtype=torch.float32, device=base.device) + 0.5) / H)[:, None].expand(H, W)
    pdf = base.max(dim=-1)[0] * torch.sin(Y * np.pi)
    pdf = pdf / pdf.sum()
    cols = torch.cumsum(pdf, dim=1)
    rows = torch.cumsum(cols[:, -1:].repeat([1, W]), dim=0)
    cols = cols / torch.where(cols[:, -1:] > 0, cols[:, -1:], torch.ones_like(cols))
    rows = rows / torch.where(rows[-1:, :] > 0, rows[-1:, :], torch.ones_like(rows))
    return pdf, rows, cols


def probe_light(lines, dev):
    gen = torch.Generator().manual_seed(1)
    base = (torch.rand(256, 256, 3, generator=gen) * 4.0 + 0.05).to(dev)
    with torch.no_grad():
        k, t = EL.tables(base), torch_tables(base)
        diffs = [float((a - b).abs().max() / b.abs().max()) for a, b in zip(k, t)]
        tk, tt = timed_pair([lambda: EL.tables(base), lambda: torch_tables(base)])
    lines += ['## 1. update_pdf, 256 x 256', '', '| what | us per call |', '|---|---|',
              f'| d3h.envlight.tables (2 launches + 4 allocations) | {fmt(tk)} |', f'| torch composition of light.py:46-59 | {fmt(tt)} |', '',
              f'Ratio of the medians: {tt[0] / tk[0]:.2f} x.  Largest relative difference between the two results: pdf {diffs[0]:.2e}, rows {diffs[1]:.2e}, '
              f'cols {diffs[2]:.2e}.', '']
    print('\n'.join(lines[-8:]), flush=True)


def probe_denoiser(lines, dev):
    lines += ['## 2. Denoiser, two images under one set of guides, sigma 2', '', '| what | size | pair: us per call | two single calls: us | ratio |', '|---|---|---|---|---|']
    verdict = True
    for res in (512, 1024):
        gen = torch.Generator().manual_seed(res)
        a, b = (torch.rand(1, res, res, 3, generator=gen).to(dev) for _ in range(2))
        nrm = torch.nn.functional.normalize(torch.tensor([0.0, 0.0, 1.0]) + 0.5 * torch.rand(1, res, res, 3, generator=gen) - 0.25, dim=-1).to(dev)
        zdz = torch.stack([2.0 + 0.2 * torch.rand(res, res, generator=gen), torch.rand(res, res, generator=gen) * 0.99 + 0.01], -1)[None].to(dev)
        with torch.no_grad():
            pa, pb = DN.bilateral_denoise_many([a, b], nrm, zdz, 2.0)
            assert torch.equal(pa, DN.bilateral_denoise(a, nrm, zdz, 2.0)) and torch.equal(pb, DN.bilateral_denoise(b, nrm, zdz, 2.0))
            tp, ts = timed_pair([lambda: DN.bilateral_denoise_many([a, b], nrm, zdz, 2.0),
                                 lambda: (DN.bilateral_denoise(a, nrm, zdz, 2.0), DN.bilateral_denoise(b, nrm, zdz, 2.0))])
        lines.append(f'| forward | {res}^2 | {fmt(tp)} | {fmt(ts)} | {ts[0] / tp[0]:.2f} x |')
        verdict &= tp[0] <= ts[0]
        la, lb = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
        oa, ob = DN.bilateral_denoise_many([la, lb], nrm, zdz, 2.0)
        sa, sb = DN.bilateral_denoise(la, nrm, zdz, 2.0), DN.bilateral_denoise(lb, nrm, zdz, 2.0)
        g = torch.randn_like(oa)
        pair = lambda: torch.autograd.grad([oa, ob], [la, lb], [g, g], retain_graph=True)
        single = lambda: (torch.autograd.grad(sa, [la], g, retain_graph=True), torch.autograd.grad(sb, [lb], g, retain_graph=True))
        assert all(torch.equal(x, y[0]) for x, y in zip(pair(), single()))
        tp, ts = timed_pair([pair, single])
        lines.append(f'| backward | {res}^2 | {fmt(tp)} | {fmt(ts)} | {ts[0] / tp[0]:.2f} x |')
        verdict &= tp[0] <= ts[0]
        print('\n'.join(lines[-2:]), flush=True)
    lines += ['', 'Each image of the pair equals the single-image call bit for bit, forward and backward (asserted above at both sizes).',
              f"**Verdict: the pair is {'no slower than' if verdict else 'SLOWER than'} two single calls in {'every' if verdict else 'at least one'} row: shade_lit "
              f"{'keeps' if verdict else 'must drop'} forward_many.**", '']
    return verdict


def _scene(a, dev):
    from d3h import scene
    return scene.Scene(device=dev, res=a.res, grid_n=a.grid, n_frames=a.frames, loss_set='full', prefit_steps=a.prefit, visualize_watertight=True,
                       flags_hook=lambda F: setattr(F, 'prefit_with_library_path', True))


def _stepper(sc, lit):
    from render import light
    from denoiser.denoiser import BilateralDenoiser
    dev = sc.device
    lgt = light.create_trainable_env_rnd(256, scale=0.0, bias=0.5) if lit else None
    den = BilateralDenoiser(influence=1.0) if lit else None
    F = sc.FLAGS

    def step():
        F.lit_shading = lit
        if lit:
            F.n_samples, F.decorrelated, F.denoiser_demodulate = 4, False, True
            lgt.base.grad = None
            lgt.update_pdf()
        bg = torch.rand(sc.n_frames, sc.res, sc.res, 3, device=dev)
        sc._zero_grad()
        r = sc.geometry.tick_init(sc.glctx, sc.target(bg), lgt, sc.material, sc.loss_fn, sc.it, den)
        total = r['d3h_total'] if 'd3h_total' in r else r['reg_loss'] + r['normal_loss'] + r['msk_loss'] + r.get('ssim_loss', 0.0)
        if lit:
            total = total + r['img_loss']          # the lit fit reads the image loss (train.py:718)
        total.backward()
        sc._optimizer_step()
        sc.it += 1
        return r
    return step


def probe_step(lines, a, dev):
    sc = _scene(a, dev)
    lit, unlit = _stepper(sc, True), _stepper(sc, False)
    r = lit()
    assert all(bool(torch.isfinite(v).all()) for v in r.values() if torch.is_tensor(v))
    tl, tu = timed_pair([lit, unlit], k=1)
    lines += [f"## 3. One tick_init step, tet grid {a.grid} (resolution {2 * a.grid + 2}), {a.res}^2, {a.frames} frames, full loss stack", '', '| what | ms per step |', '|---|---|',
              f"| FLAGS.lit_shading, bsdf 'pbr', n_samples 4, BilateralDenoiser(1.0) (sigma 2), update_pdf at 256^2 included | "
              f'{tl[0] / 1e3:.2f} ({tl[1] / 1e3:.2f}-{tl[2] / 1e3:.2f}) |', f"| flag off: the 'kd' path of the parent commit | {tu[0] / 1e3:.2f} ({tu[1] / 1e3:.2f}-{tu[2] / 1e3:.2f}) |", '']
    print('\n'.join(lines[-6:]), flush=True)


def _short(name):
    import re
    m = re.search(r'(\w+(?:<[^>]*>)?)\(', name.replace('(anonymous namespace)::', ''))
    return m.group(1) if m else name[:60]


def trace_child(a):
    """run by the parent under rocprofv3: a few steps of one kind"""
    dev = 'cuda'
    sc = _scene(a, dev)
    step = _stepper(sc, a.trace_child == 'lit')
    step()                                                     # warm-up, with the start-up (SDF pre-fit) before it
    torch.cuda.synchronize()
    EL.tables(torch.ones(MARK_ROWS, 5, 3, device=dev))          # a marker in the trace: everything after this dispatch is the timed steps
    for _ in range(a.trace_steps):
        step()
    torch.cuda.synchronize()


def probe_trace(lines, a):
    for kind in ('lit', 'unlit'):
        d = os.path.join(a.trace_dir, kind)
        cmd = ['rocprofv3', '--kernel-trace', '--stats', '-d', d, '-o', 'step', '--output-format', 'csv', '--', sys.executable, os.path.abspath(__file__), '--trace-child', kind,
               '--res', str(a.res), '--grid', str(a.grid), '--frames', str(a.frames), '--prefit', str(a.prefit), '--trace-steps', str(a.trace_steps)]
        try:
            rc = subprocess.call(cmd, stdout=subprocess.DEVNULL, timeout=900)
        except subprocess.TimeoutExpired:
            rc = 'timeout'
        lines += [f'### Kernels of one {kind} step: mean over {a.trace_steps} steps after a warm-up step (rocprofv3 --kernel-trace; top 14 by time)', '']
        if rc != 0:
            # the child may have aborted, faulted or hung on the card: nothing more is started on it by this probe
            lines += [f'not measured: the traced child ended with {rc}; the probe stopped there', '']
            return
        files = glob.glob(os.path.join(d, '**', '*kernel_trace.csv'), recursive=True)
        if not files:
            lines += ['not measured: rocprofv3 left no kernel trace', '']
            continue
        disp = sorted(csv.DictReader(open(files[0])), key=lambda r_: int(r_['Start_Timestamp']))
        mark = [i for i, r_ in enumerate(disp) if 'envlight_row_kernel' in r_['Kernel_Name'] and int(r_['Grid_Size_X']) == MARK_ROWS * 256]
        if not mark:
            lines += ['not measured: the marker dispatch is not in the trace', '']
            continue
        agg = {}
        for r_ in disp[mark[-1] + 2:]:                           # past the marker's two launches
            e = agg.setdefault(r_['Kernel_Name'], [0, 0.0])
            e[0] += 1
            e[1] += int(r_['End_Timestamp']) - int(r_['Start_Timestamp'])
        rows = [{'Name': k, 'Calls': v[0] / a.trace_steps, 'TotalDurationNs': v[1] / a.trace_steps} for k, v in agg.items()]
        rows.sort(key=lambda r_: -r_['TotalDurationNs'])
        total = sum(r_['TotalDurationNs'] for r_ in rows)
        lines += [f'Sum of kernel times per step: {total / 1e6:.2f} ms in {sum(r_["Calls"] for r_ in rows):.0f} launches (kernels of different streams overlap: the sum '
                  f'is not the step time).', '', '| kernel | launches per step | ms per step | mean us | share of the sum |', '|---|---|---|---|---|']
        for r_ in rows[:14]:
            t = r_['TotalDurationNs']
            lines.append(f"| `{r_['Name'][:90]}` | {r_['Calls']:.1f} | {t / 1e6:.3f} | {t / 1e3 / r_['Calls']:.1f} | {100.0 * t / total:.1f} % |")
        mine = [r_ for r_ in rows if any(s_ in r_['Name'] for s_ in ('envlight', 'denoise', 'env_shade', 'bvh_'))]
        lines += ['', 'Kernels of the lit branch per step: ' + ('none' if not mine else '; '.join(
            f"`{_short(r_['Name'])}` {r_['Calls']:.1f} x {r_['TotalDurationNs'] / 1e3 / r_['Calls']:.1f} us" for r_ in mine)), '']
        print('\n'.join(lines[-20:]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'lit_probe.md'))
    ap.add_argument('--commit', default='working tree')
    ap.add_argument('--res', type=int, default=1024)
    ap.add_argument('--grid', type=int, default=63)
    ap.add_argument('--frames', type=int, default=4)
    ap.add_argument('--prefit', type=int, default=300)
    ap.add_argument('--no-trace', action='store_true')
    ap.add_argument('--no-step', action='store_true')
    ap.add_argument('--trace-dir', default=os.path.join(ROOT, 'build', 'lit_trace'))          # build/ is ignored by git: traces are not committed
    ap.add_argument('--trace-steps', type=int, default=3)
    ap.add_argument('--trace-child', default=None)
    a = ap.parse_args()
    if a.trace_child:
        return trace_child(a)
    dev = 'cuda'
    lines = ['# The lit render path: light tables, two-image denoiser, one lit tick_init step (tools/gpu_probe_lit.py)', '',
             f'Commit: {a.commit}.  GPU: {torch.cuda.get_device_name(0)}.  Per-call median (min-max) over {REPS} windows timed with device events; the two '
             f'variants of a row alternate window by window.  No test asserts a time.', '']
    probe_light(lines, dev)
    probe_denoiser(lines, dev)
    if not a.no_step:
        probe_step(lines, a, dev)
        if not a.no_trace:
            probe_trace(lines, a)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, 'w').write('\n'.join(lines) + '\n')
    print(f'wrote {a.out}')


if __name__ == '__main__':
    assert torch.cuda.is_available(), 'needs the GPU'
    main()
