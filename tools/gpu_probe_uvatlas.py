"""Times of the textured-mesh export on the GPU, beside the reference's route on the same atlas.

    python tools/gpu_probe_uvatlas.py [--out FILE.md] [--commit TEXT] [--faces 200000] [--res 2048]      # default profiles/uvatlas_probe.md

 1. d3h.uvatlas.make_atlas, d3h.uvatlas.bake_positions and MLPTexture3D.sample(pos, mask=owned) (the reference-shaped texture: the fused kernel of
    csrc/texmlp.hip) on a random soup of --faces triangles inside the texture's box at --res x --res -- the three steps of d3h.export.textured_mesh.
 2. The reference's route on the SAME atlas: render.render.render_uv (rasterise the chart, interpolate positions, sample the MLP on every texel)
    followed by the two util.dilate(.., 7) calls of train.py:221-225.
 3. VGPRs, scratch, LDS and occupancy of the kernels of csrc/uvatlas.hip, from hipcc -Rpass-analysis=kernel-resource-usage where hipcc is at hand.

Timing: every entry is warmed up (3 calls); then 10 windows are timed with device events, each window as many back-to-back calls as make it last
about 20 ms; the table gives the per-call median and the min-max spread.  These are records, not gates: no test asserts any of them."""
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
sys.path.insert(0, PKG)
from d3h import build as B, uvatlas as UA          # noqa: E402

REPS = 10


def _window(fn, k):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(k):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / k


def timed(fn, reps=REPS, window_us=20000.0):
    """-> (median, min, max) in us per call"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    k = max(1, min(200, int(window_us / max(_window(fn, 1), 1.0))))
    ts = [_window(fn, k) for _ in range(reps)]
    return statistics.median(ts), min(ts), max(ts)


def resource_rows(lines):
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    lines += ['## Kernel resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950)', '']
    if not os.path.exists(hipcc):
        lines += ['not collected: no hipcc on this machine', '']
        return
    lines += ['| kernel | VGPRs | SGPRs | scratch bytes / lane | LDS bytes / block | waves / SIMD |', '|---|---|---|---|---|---|']
    cmd = [hipcc] + [x for x in B.FLAGS if x != '-shared'] + ['-Rpass-analysis=kernel-resource-usage', '-c', os.path.join(B.CSRC, 'uvatlas.hip'), '-o', os.devnull, '-I', B.CSRC]
    txt = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT).stdout.decode()
    demangle = lambda s: subprocess.run(['c++filt', s], stdout=subprocess.PIPE).stdout.decode().strip() if os.path.exists('/usr/bin/c++filt') else s
    for blk in txt.split('Function Name: ')[1:]:
        get = lambda k: re.search(k + r': (\d+)', blk).group(1)
        name = re.sub(r'\(anonymous namespace\)::|\(.*', '', demangle(blk.split()[0]))
        row = f'| {name} | ' + ' | '.join(get(k) for k in ('VGPRs', 'TotalSGPRs', r'ScratchSize \[bytes/lane\]', r'LDS Size \[bytes/block\]', r'Occupancy \[waves/SIMD\]')) + ' |'
        lines.append(row)
        print(row, flush=True)
    lines.append('')


def main(dev='cuda'):
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'uvatlas_probe.md'))
    ap.add_argument('--commit', default=None)
    ap.add_argument('--faces', type=int, default=200000)
    ap.add_argument('--res', type=int, default=2048)
    a = ap.parse_args()
    commit = a.commit
    if commit is None:
        try:
            commit = subprocess.check_output(['git', '-C', ROOT, 'rev-parse', '--short', 'HEAD'], stderr=subprocess.DEVNULL).decode().strip()
        except Exception:
            commit = 'unknown'
    import nvdiffrast.torch as dr
    from render import mesh as rmesh, mlptexture, render as rrender, util
    F, R = a.faces, a.res
    rng = np.random.default_rng(1)
    centre = rng.uniform((-0.7, -1.1, -0.15), (0.5, 0.5, 0.15), (F, 1, 3))
    v = torch.tensor((centre + rng.uniform(-0.01, 0.01, (F, 3, 3))).reshape(-1, 3), dtype=torch.float32, device=dev)
    t = torch.arange(3 * F, device=dev).reshape(F, 3)
    lo, hi = torch.tensor([0, 0, 0, 0, 0.001, 0.0], device=dev), torch.tensor([1, 1, 1, 0, 1.0, 1.0], device=dev)
    mlp = mlptexture.MLPTexture3D((v.min(0).values, v.max(0).values), channels=6, min_max=[lo, hi])
    atlas = UA.make_atlas(v, t, R)
    pos, owned, inside, _ = UA.bake_positions(atlas, v, t)
    m = rmesh.Mesh(v, t, v_tex=atlas.uvs, t_tex_idx=atlas.t_tex_idx)
    ctx = dr.RasterizeGLContext()
    lines = [f'# Textured-mesh export probe ({commit}; {torch.cuda.get_device_name(0)})', '',
             f'{F} triangles, {R} x {R} texture: cells of s = {atlas.s} texels ({atlas.nx} x {atlas.ny}), {int(owned.sum())} owned texels, {int(inside.sum())} inside a triangle '
             f'(efficiency (s-4)^2/s^2 = {(atlas.s - 4) ** 2 / atlas.s ** 2:.2f} of a cell).', '',
             '| step | median us | min | max |', '|---|---|---|---|']

    def row(name, fn):
        med, mn, mx = timed(fn)
        lines.append(f'| {name} | {med:.1f} | {mn:.1f} | {mx:.1f} |')
        print(lines[-1], flush=True)
        return med

    with torch.no_grad():
        ours = row('make_atlas (1 launch)', lambda: UA.make_atlas(v, t, R))
        ours += row('bake_positions (1 launch)', lambda: UA.bake_positions(atlas, v, t))
        ours += row('MLPTexture3D.sample(pos, mask=owned)', lambda: mlp.sample(pos, mask=owned))
        ref = row('reference route: render_uv (rasterise + interpolate + sample every texel)', lambda: rrender.render_uv(ctx, m, [R, R], mlp))
        cover, kd, ks = rrender.render_uv(ctx, m, [R, R], mlp)
        avg = torch.zeros(1, 1, 1, 3, device=dev)
        ref += row('reference route: two util.dilate(.., 7)', lambda: (util.dilate(kd, avg, cover, 7), util.dilate(ks, avg, cover, 7)))
    lines += ['', f'Sum of the medians: this build {ours:.0f} us, the reference route on the same atlas {ref:.0f} us.', '']
    resource_rows(lines)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print('wrote', a.out)


if __name__ == '__main__':
    main()
