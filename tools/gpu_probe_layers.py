"""Times of the layered render (depth-peeled layers blended back to front) on the GPU: the fused blend step against the composed route.

    python tools/gpu_probe_layers.py [--out FILE.md] [--commit TEXT] [--sub 6] [--shells 4] [--layers 4] [--tex 2048] [--res 1024] [--frames 4]     # default profiles/layers_probe.md

Scene: --shells concentric synth.icosphere(--sub) shells in one mesh (4 x 32768 = 131072 triangles at the defaults, the size of a fitted mesh of the
training scene), exported with d3h.export.textured_mesh(transparency=True), the position as colour and a smooth opacity in [0.2, 0.9];
render.render.render_mesh(num_layers=--layers) under FLAGS.transparency of --frames views at --res x --res under fixed random draws.  Two routes for
the blend of the shaded layers, everything else (peeling, G-buffer, lookups, shading) being the same code:
  (a) fused     D3H_LAYER_FUSED=1: d3h.imgops.layer_composite_antialias, one launch per layer each way (csrc/raster.hip: layer_composite_*_kernel)
  (b) composed  D3H_LAYER_FUSED=0: torch.cat of the sources, torch.lerp and nvdiffrast.antialias per layer
with all buffers and with buffers=('shaded',), forward (under torch.no_grad()) and forward + backward (gradients of the three maps for a fixed output
gradient).  Both routes are run on the same inputs and their results compared before anything is timed.

Timing: 3 warm-up calls each; then 10 rounds, each round one window of (a) and one of (b) in turn (device events around as many back-to-back calls as
make the window last about 100 ms); per-call median and min-max over the rounds.  The run-to-run spread of a figure is (max - min) / median.  Rule for
the default of render.render (LAYER_FUSED_DEFAULT): fused only if its forward + backward median with all buffers beats the composed one by more than
the larger of the two spreads; otherwise opt-in behind D3H_LAYER_FUSED=1.  The file says which happened.  These are times of whole render_mesh
calls: the blend is a part of them."""
import argparse
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'd3human-code_amd')
sys.path.insert(0, PKG)

ROUNDS = 10
WINDOW_US = 100000.0


def _window(fn, k):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(k):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / k


def timed_pair(fa, fb):
    """-> ((median, min, max) of fa, the same of fb) in us per call, the windows of the two alternating"""
    ks = []
    for fn in (fa, fb):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ks.append(max(1, min(500, int(WINDOW_US / max(_window(fn, 1), 1.0)))))
    ta, tb = [], []
    for _ in range(ROUNDS):
        ta.append(_window(fa, ks[0]))
        tb.append(_window(fb, ks[1]))
    return tuple((statistics.median(t), min(t), max(t)) for t in (ta, tb))


class _Flags:
    transparency = True


def main(dev='cuda', timer=timed_pair, argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'layers_probe.md'))
    ap.add_argument('--commit', default=None)
    ap.add_argument('--sub', type=int, default=6)
    ap.add_argument('--shells', type=int, default=4)
    ap.add_argument('--layers', type=int, default=4)
    ap.add_argument('--tex', type=int, default=2048)
    ap.add_argument('--res', type=int, default=1024)
    ap.add_argument('--frames', type=int, default=4)
    a = ap.parse_args(argv)
    commit = a.commit
    if commit is None:
        try:
            commit = subprocess.check_output(['git', '-C', ROOT, 'rev-parse', '--short', 'HEAD'], stderr=subprocess.DEVNULL).decode().strip()
        except Exception:
            commit = 'unknown'
    import numpy as np
    import nvdiffrast.torch as dr
    from d3h import export, synth
    from render import mesh as rmesh, render as rr, util

    class PositionAsColour:
        def sample(self, p, *args, **kw):
            return torch.cat((p, p), dim=-1)

    v, t = synth.icosphere(a.sub)
    v, t = np.asarray(v, np.float32), np.asarray(t, np.int64)
    radii = [0.6 * (1.0 - 0.5 * k / max(a.shells, 1)) for k in range(a.shells)]
    vv = torch.as_tensor(np.concatenate([v * np.float32(r) for r in radii]), dtype=torch.float32, device=dev)
    tt = torch.as_tensor(np.concatenate([t + k * len(v) for k in range(a.shells)]), dtype=torch.int64, device=dev)
    mat = {'bsdf': 'pbr', 'kd_ks': PositionAsColour()}
    base = rmesh.auto_normals(rmesh.Mesh(vv, tt, material=mat))
    ex = rmesh.compute_tangents(export.textured_mesh(base, mat, a.tex, [-1.0] * 3, [1.0] * 3, [-1.0] * 3, [1.0] * 3, [-1.0, -1.0, 0.0], [1.0, 1.0, 1.0],
                                                     transparency=True))
    with torch.no_grad():
        y, x = torch.meshgrid(torch.arange(a.tex, dtype=torch.float32) / a.tex, torch.arange(a.tex, dtype=torch.float32) / a.tex, indexing='ij')
        ex.material['kd'].data[..., 3] = (0.55 + 0.35 * torch.sin(7.0 * x + 1.0) * torch.cos(5.0 * y)).to(dev)
    R, NB = a.res, a.frames
    proj = util.perspective(0.6, 1.0, 0.1, 10.0)
    mvp = torch.stack([proj @ util.translate(0.0, 0.0, -1.9) @ util.rotate_y(0.7 * b + 0.3) @ util.rotate_x(0.2) for b in range(NB)]).to(dev)
    cam = torch.stack([torch.linalg.inv(util.translate(0.0, 0.0, -1.9) @ util.rotate_y(0.7 * b + 0.3) @ util.rotate_x(0.2))[:3, 3] for b in range(NB)]).to(dev)
    gen = torch.Generator().manual_seed(3)
    draws = {'noise': torch.randn(NB, R, R, 3, generator=gen).to(dev), 'offset': (torch.randn(NB, R, R, 2, generator=gen) * 0.005).to(dev),
             'pos_noise': (torch.randn(NB, R, R, 3, generator=gen) * 0.01).to(dev)}
    maps = [ex.material[k].data for k in ('kd', 'ks', 'normal')]
    ctx = dr.RasterizeGLContext()

    def run(fused, buffers):
        old = os.environ.get('D3H_LAYER_FUSED')
        os.environ['D3H_LAYER_FUSED'] = '1' if fused else '0'
        try:
            return rr.render_mesh(_Flags(), 0, ctx, ex, None, mvp, cam, None, [R, R], num_layers=a.layers, _rng_draws=draws, buffers=buffers)
        finally:
            if old is None:
                del os.environ['D3H_LAYER_FUSED']
            else:
                os.environ['D3H_LAYER_FUSED'] = old

    with torch.no_grad():
        first = run(True, ('shaded', '_rast'))
        covered = int((first['_rast'][..., 3] > 0).sum())
    lines = [f'# Layered render probe ({commit}; {torch.cuda.get_device_name(0) if dev == "cuda" else dev})', '',
             f'{tt.shape[0]} triangles in {a.shells} shells, maps of {a.tex} x {a.tex}, {NB} frames of {R} x {R}, {a.layers} layers: {covered} pixels of {NB * R * R} '
             f'covered by the first layer.  Times of whole render_mesh calls, us.', '']
    res = {}
    for what, buffers in (('all buffers', None), ("('shaded',)", ('shaded',))):
        key = 'shaded' if buffers else '_stacked'
        gs = None

        def loss_grads(fused):
            out = run(fused, buffers)[key]
            return torch.autograd.grad(out, maps, gs, allow_unused=True)
        with torch.no_grad():
            fa, fb = run(True, buffers)[key], run(False, buffers)[key]
        gs = (torch.rand(fa.shape, generator=gen) + 0.5).to(dev)
        ga, gb = loss_grads(True), loss_grads(False)
        d_out = float((fa - fb).abs().max())
        d_grad = max(float((x_ - y_).abs().max() / y_.abs().max().clamp(min=1e-30)) for x_, y_ in zip(ga, gb) if x_ is not None)
        note = '' if buffers else (' -- the first pass of 12 buffers, which is what the backward differentiates; perturbed_nrm_grad goes '
                                   'through a second pass of 4 channels that is rendered in both windows and not differentiated')
        lines += [f'## {what} ({fa.shape[-1]} channels{note})', '',
                  f'Fused against composed on these inputs: images differ by at most {d_out:.2e}, map gradients by {d_grad:.2e} of their largest entry.', '',
                  '| pass | fused median us | min | max | composed median us | min | max |', '|---|---|---|---|---|---|---|']
        with torch.no_grad():
            res[what, 'forward'] = timer(lambda: run(True, buffers), lambda: run(False, buffers))
        res[what, 'forward + backward'] = timer(lambda: loss_grads(True), lambda: loss_grads(False))
        for k in ('forward', 'forward + backward'):
            x_, y_ = res[what, k]
            lines.append(f'| {k} | {x_[0]:.1f} | {x_[1]:.1f} | {x_[2]:.1f} | {y_[0]:.1f} | {y_[1]:.1f} | {y_[2]:.1f} |')
            print(what, lines[-1], flush=True)
        (fa_med, fa_min, fa_max), (fb_med, fb_min, fb_max) = res[what, 'forward + backward']
        lines += ['', f'Run-to-run spread of forward + backward, (max - min) / median: fused {(fa_max - fa_min) / fa_med:.1%}, composed {(fb_max - fb_min) / fb_med:.1%}.  '
                  f'Forward + backward: fused {fa_med:.1f} us against composed {fb_med:.1f} us, {fb_med / fa_med:.2f} x.', '']
    (fa_med, fa_min, fa_max), (fb_med, fb_min, fb_max) = res['all buffers', 'forward + backward']
    spread = max((fa_max - fa_min) / fa_med, (fb_max - fb_min) / fb_med)
    wins = fa_med < fb_med * (1.0 - spread)
    lines += ['**Outcome: ' + ('with all buffers the fused blend beats the composed route by more than the spread: it is the default (LAYER_FUSED_DEFAULT = True; '
                               'D3H_LAYER_FUSED=0 switches it off).' if wins else
                               'with all buffers the fused blend does not beat the composed route by more than the spread: it is opt-in behind D3H_LAYER_FUSED=1 '
                               '(LAYER_FUSED_DEFAULT = False).') + '**', '']
    print('\n'.join(lines[-2:]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print('wrote', a.out)


if __name__ == '__main__':
    main()
