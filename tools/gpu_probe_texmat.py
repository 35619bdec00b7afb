"""Times of the per-pixel material lookup of a textured mesh on the GPU: the fused pass against the composed route.

    python tools/gpu_probe_texmat.py [--out FILE.md] [--commit TEXT] [--sub 7] [--tex 2048] [--res 1024] [--frames 4]     # default profiles/texmat_probe.md

Scene: d3h.export.textured_mesh of synth.icosphere(--sub) (8 * 4^sub triangles; 131072 at the default, the size of a fitted mesh of the training
scene) with the position as colour, maps --tex x --tex, one rasterisation of --frames views at --res x --res, kept fixed.  Two routes to the three
images (kd, ks, normal), forward and backward (gradients of the three maps for a fixed output gradient, zero at uncovered pixels):
  (a) fused     d3h.texmat.lookup: one launch each way (csrc/texmat.hip)
  (b) composed  nvdiffrast.interpolate of v_tex + three nvdiffrast.texture(filter_mode='linear', boundary_mode='wrap'): the ops of the parent commit
Both are run on the same inputs and their results compared before anything is timed.

Timing: 3 warm-up calls each; then 10 rounds, each round one window of (a) and one of (b) in turn (device events around as many back-to-back calls as
make the window last about 50 ms); per-call median and min-max over the rounds.  The run-to-run spread of a figure is (max - min) / median.  Rule for
the default of render.render (TEXMAT_FUSED_DEFAULT): fused only if its forward + backward median beats the composed one by more than the larger of
the two spreads; otherwise opt-in behind D3H_TEXMAT_FUSED=1.  The file says which happened.  The backward's atomic traffic: covered pixels x 4 taps x
9 channels x 4 bytes, over the backward's time (to be read against the chip-wide float-atomic rate of about 1.3 TB/s of added bytes)."""
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
WINDOW_US = 50000.0


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


def main(dev='cuda', timer=timed_pair):
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'texmat_probe.md'))
    ap.add_argument('--commit', default=None)
    ap.add_argument('--sub', type=int, default=7)
    ap.add_argument('--tex', type=int, default=2048)
    ap.add_argument('--res', type=int, default=1024)
    ap.add_argument('--frames', type=int, default=4)
    a = ap.parse_args()
    commit = a.commit
    if commit is None:
        try:
            commit = subprocess.check_output(['git', '-C', ROOT, 'rev-parse', '--short', 'HEAD'], stderr=subprocess.DEVNULL).decode().strip()
        except Exception:
            commit = 'unknown'
    import nvdiffrast.torch as dr
    from d3h import export, synth, texmat
    from render import mesh as rmesh, renderutils as ru, util

    class PositionAsColour:
        def sample(self, p, *args, **kw):
            return torch.cat((p, p), dim=-1)

    v, t = synth.icosphere(a.sub)
    v, t = torch.as_tensor(v, dtype=torch.float32, device=dev) * 0.6, torch.as_tensor(t, dtype=torch.int64, device=dev)
    mat = {'bsdf': 'pbr', 'kd_ks': PositionAsColour()}
    ex = export.textured_mesh(rmesh.Mesh(v, t, material=mat), mat, a.tex, [-1.0] * 3, [1.0] * 3, [-1.0] * 3, [1.0] * 3, [-1.0, -1.0, 0.0], [1.0, 1.0, 1.0])
    R, NB = a.res, a.frames
    proj = util.perspective(0.6, 1.0, 0.1, 10.0)
    mvp = torch.stack([proj @ util.translate(0.0, 0.0, -1.9) @ util.rotate_y(0.7 * b) for b in range(NB)]).to(dev)
    clip = ru.xfm_points(v[None], mvp)
    with torch.no_grad():
        rast, _ = dr.rasterize(dr.RasterizeGLContext(), clip, t.int(), [R, R])
    covered = int((rast[..., 3] > 0).sum())
    maps = [ex.material[k].data for k in ('kd', 'ks', 'normal')]
    v_tex, tri = ex.v_tex.contiguous(), ex.t_tex_idx.int().contiguous()
    gen = torch.Generator().manual_seed(3)
    gs = [(torch.rand(NB, R, R, 3, generator=gen) + 0.5).to(dev) for _ in maps]

    def fused_fwd():
        return texmat.lookup(rast, v_tex, tri, maps, boundary='wrap')

    def composed_fwd():
        texc, _ = dr.interpolate(v_tex[None], rast, tri)
        return [dr.texture(m, texc, filter_mode='linear', boundary_mode='wrap') for m in maps]

    # the same results first (the composed route reads texel (0, 0) at empty pixels: compared where covered)
    hit = (rast[..., 3:4] > 0).float()
    gs = [g * hit for g in gs]                      # (as in render_mesh, where an uncovered pixel passes no gradient back)
    fa, fb = fused_fwd(), composed_fwd()
    ga, gb = torch.autograd.grad(fa, maps, gs), torch.autograd.grad(fb, maps, gs)
    d_out = max(float(((x - y) * hit).detach().abs().max()) for x, y in zip(fa, fb))
    d_grad = max(float((x - y).abs().max() / y.abs().max().clamp(min=1e-30)) for x, y in zip(ga, gb))
    lines = [f'# Per-pixel material lookup probe ({commit}; {torch.cuda.get_device_name(0) if dev == "cuda" else dev})', '',
             f'{t.shape[0]} triangles, three {a.tex} x {a.tex} x 3 maps, {NB} frames of {R} x {R}: {covered} covered pixels of {NB * R * R}.',
             f'Fused against composed on these inputs: images differ by at most {d_out:.2e} (covered pixels), map gradients by {d_grad:.2e} of their largest entry '
             f'(the atomics add in another order).', '',
             '| pass | fused median us | min | max | composed median us | min | max |', '|---|---|---|---|---|---|---|']
    out_a, out_b = fused_fwd(), composed_fwd()
    res = {}
    with torch.no_grad():
        res['forward'] = timer(fused_fwd, composed_fwd)
    res['backward'] = timer(lambda: torch.autograd.grad(out_a, maps, gs, retain_graph=True), lambda: torch.autograd.grad(out_b, maps, gs, retain_graph=True))
    res['forward + backward'] = timer(lambda: torch.autograd.grad(fused_fwd(), maps, gs), lambda: torch.autograd.grad(composed_fwd(), maps, gs))
    for k, (x, y) in res.items():
        lines.append(f'| {k} | {x[0]:.1f} | {x[1]:.1f} | {x[2]:.1f} | {y[0]:.1f} | {y[1]:.1f} | {y[2]:.1f} |')
        print(lines[-1], flush=True)
    (fa_med, fa_min, fa_max), (fb_med, fb_min, fb_max) = res['forward + backward']
    spread = max((fa_max - fa_min) / fa_med, (fb_max - fb_min) / fb_med)
    wins = fa_med < fb_med * (1.0 - spread)
    atomic_bytes = covered * 4 * 9 * 4
    bwd_a, bwd_b = res['backward'][0][0], res['backward'][1][0]
    lines += ['', f'Run-to-run spread of forward + backward, (max - min) / median: fused {(fa_max - fa_min) / fa_med:.1%}, composed {(fb_max - fb_min) / fb_med:.1%}.',
              f'Forward + backward: fused {fa_med:.1f} us against composed {fb_med:.1f} us, {fb_med / fa_med:.2f} x.',
              f'Backward atomics: {atomic_bytes / 1e6:.1f} MB of added bytes; fused {atomic_bytes / bwd_a / 1e6:.3f} TB/s, composed {atomic_bytes / bwd_b / 1e6:.3f} TB/s '
              f'(12-byte segments per tap and map).', '',
              '**Outcome: ' + ('the fused pass beats the composed route by more than the spread: it is the default (TEXMAT_FUSED_DEFAULT = True; D3H_TEXMAT_FUSED=0 '
                               'switches it off).' if wins else
                               'the fused pass does not beat the composed route by more than the spread: it is opt-in behind D3H_TEXMAT_FUSED=1 '
                               '(TEXMAT_FUSED_DEFAULT = False).') + '**', '']
    print('\n'.join(lines[-6:]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print('wrote', a.out)


if __name__ == '__main__':
    main()
