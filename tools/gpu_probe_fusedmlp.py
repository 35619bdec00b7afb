"""Stand-alone times and peak memory of the general fused MLP (csrc/fusedmlp.hip) beside the library-GEMM composition it replaces.

    python tools/gpu_probe_fusedmlp.py [--rows N] [--out FILE.md]          # defaults 4 x 1024^2, profiles/fusedmlp_probe.md

Three shapes, each ReLU inside: 32 -> 32 -> 32 -> 6 with the sigmoid range map and the x128 input-gradient scale (the 16-level texture of
render/mlptexture.py), 32 -> 64 x 3 -> 9 and 20 -> 128 x 5 -> 16.  Each is measured
  * fused: d3h.fusedmlp.fused_mlp (one kernel forward, one backward, no activation kept), and
  * library: the composition MLPTexture3D._sample_composed runs with D3H_TEX_FUSED_NET=0 -- _ScaleGrad, one torch.nn.functional.linear and
    one ReLU per layer, the sigmoid and the range map -- under autograd, which keeps every hidden activation,
on the same inputs: the forward alone (no graph), forward + backward (gradients for x and every matrix), and the peak of
torch.cuda.max_memory_allocated over one forward + backward above what is allocated before it.  The two floors per row are computed from
the shapes: the compulsory bytes (x and out forward; x, out, g_out and d_x on top for forward + backward) at 8 TB/s, and the FLOP
(2 N sum(fan_in fan_out) forward, three times that with both gradients) at the 157 TF peak of the f32 matrix instruction.

Timing: 3 warm-ups per variant, then REPS rounds in which the two variants ALTERNATE in one process, each run timed with device events;
the table reports the median and the min-max spread.  The buffers (0.3 - 0.5 GB each) are larger than the 256 MiB Infinity Cache."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'd3human-code_amd'))
from d3h import fusedmlp                                  # noqa: E402
from render.mlptexture import _ScaleGrad                  # noqa: E402

REPS = 10
HBM_BPS, MFMA_F32_FLOPS = 8e12, 157e12
SHAPES = [('32 -> 32 -> 32 -> 6, sigmoid range map, x128', (32, 32, 2, 6), 'Sigmoid', True),
          ('32 -> 64 x 3 -> 9', (32, 64, 3, 9), 'None', False),
          ('20 -> 128 x 5 -> 16', (20, 128, 5, 16), 'None', False)]


def event_time(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3        # us


def alternated(fns, reps=REPS):
    """[(median, min, max)] per variant: 3 warm-ups each, then `reps` rounds running the variants one after the other"""
    for fn in fns:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            ts[k].append(event_time(fn))
    return [(statistics.median(t), min(t), max(t)) for t in ts]


def fmt(t):
    return f'{t[0]:.0f} ({t[1]:.0f}-{t[2]:.0f})'


def peak_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def probe(label, shape, out_act, texture, n, dev, lines):
    n_in, width, hidden, n_out = shape
    cfg = fusedmlp.MLPConfig(n_in, n_out, {'otype': 'FullyFusedMLP', 'activation': 'ReLU', 'output_activation': out_act, 'n_neurons': width,
                                           'n_hidden_layers': hidden})
    gen = torch.Generator().manual_seed(0)
    ws = [(((torch.rand(fo, fi, generator=gen) * 2 - 1) * (6.0 / (fi + fo)) ** 0.5).to(dev)).requires_grad_(True) for fo, fi in cfg.shapes]
    x = (torch.rand(n, n_in, generator=gen) * 2 - 1).to(dev).requires_grad_(True)
    G = torch.randn(n, n_out, generator=gen).to(dev)
    lo, hi = (torch.rand(n_out, generator=gen) * 0.1).to(dev), (0.5 + torch.rand(n_out, generator=gen)).to(dev)
    scale = 128.0 if texture else 1.0

    def fused():
        return fusedmlp.fused_mlp(x, ws, cfg, out_scale=(hi - lo) if texture else None, out_bias=lo if texture else None, in_grad_scale=scale)

    def library():
        h = _ScaleGrad.apply(x, scale) if texture else x
        for w in ws[:-1]:
            h = torch.relu(torch.nn.functional.linear(h, w))
        o = torch.nn.functional.linear(h, ws[-1])
        if texture:
            o = torch.sigmoid(o) * (hi[None, :] - lo[None, :]) + lo[None, :]
        return o

    def fwd_only(f):
        def run():
            with torch.no_grad():
                f()
        return run

    def fwd_bwd(f):
        def run():
            x.grad = None
            for w in ws:
                w.grad = None
            (f() * G).sum().backward()
        return run

    with torch.no_grad():
        diff = float((fused() - library()).abs().max())
    t_f = alternated([fwd_only(fused), fwd_only(library)])
    t_fb = alternated([fwd_bwd(fused), fwd_bwd(library)])
    mem = [peak_mb(fwd_bwd(fused)), peak_mb(fwd_bwd(library))]
    flop = 2.0 * n * sum(a * b for a, b in cfg.shapes)
    by_f, by_fb = 4.0 * n * (n_in + n_out), 4.0 * n * (3 * n_in + 2 * n_out)
    for k, name in enumerate(('fused (csrc/fusedmlp.hip)', 'library GEMMs (the D3H_TEX_FUSED_NET=0 composition)')):
        row = f'| {label} | {name} | {fmt(t_f[k])} | {fmt(t_fb[k])} | {mem[k]:.0f} |'
        lines.append(row)
        print(row, flush=True)
    gap, spread = t_fb[1][0] - t_fb[0][0], max(t_fb[0][2] - t_fb[0][1], t_fb[1][2] - t_fb[1][1])
    row = (f'| {label} | library / fused; the difference against the larger min-max spread | {t_f[1][0] / t_f[0][0]:.2f} | {t_fb[1][0] / t_fb[0][0]:.2f}; '
           f'{gap:.0f} us against {spread:.0f} us | {mem[1] / max(mem[0], 1e-9):.2f} |')
    lines.append(row)
    print(row, flush=True)
    row = (f'| {label} | floors: bytes at 8 TB/s; FLOP at 157 TF | {by_f / HBM_BPS * 1e6:.0f}; {flop / MFMA_F32_FLOPS * 1e6:.0f} | '
           f'{by_fb / HBM_BPS * 1e6:.0f}; {3 * flop / MFMA_F32_FLOPS * 1e6:.0f} | (largest output difference of the two: {diff:.1e}) |')
    lines.append(row)
    print(row, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=4 * 1024 * 1024)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'fusedmlp_probe.md'))
    a = ap.parse_args()
    n = a.rows
    lines = ['# General fused MLP: stand-alone times and peak memory (tools/gpu_probe_fusedmlp.py)', '',
             f'{n} rows; us per call, median of {REPS} runs timed with device events (min-max), the two variants alternated in one process after 3',
             'warm-ups each; "peak" is torch.cuda.max_memory_allocated over one forward + backward above what was allocated before it, MiB.',
             'Forward + backward computes the gradients of x and of every matrix.', '',
             '| shape | code | forward | forward + backward | peak MiB |', '|---|---|---|---|---|']
    for label, shape, out_act, texture in SHAPES:
        probe(label, shape, out_act, texture, n, 'cuda', lines)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, 'w').write('\n'.join(lines) + '\n')
    print(f'wrote {a.out}')


if __name__ == '__main__':
    assert torch.cuda.is_available(), 'needs the GPU'
    main()
