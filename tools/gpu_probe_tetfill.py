"""Times and counts of d3h.tetfill.fill_mesh (csrc/tetfill.hip) on the GPU, and the quality of its tets.

    python tools/gpu_probe_tetfill.py [--out FILE.md] [--commit TEXT] [--res 64 128]      # default profiles/tetfill_probe.md

Mesh: a closed latitude-longitude sphere of radius 0.5 with 100 x 100 cells (19 800 faces).  Per resolution:
  first call    fill_mesh with nothing cached: the lattice (host numpy, copied over), the edge tables of d3h.mtets.TetGrid (one torch.unique over
                the 6 T corner pairs), the distance field and the clip
  later calls   fill_mesh again (lattice and edge tables cached), and its two parts alone: meshops.mesh_wsdf on the lattice vertices, and
                tetfill.clip (three launches, three torch.cumsum, one read-back)
  counts        lattice vertices / tets, inside vertices, cut vertices, children
  quality       child volume relative to h^3 / 6 (the volume of an uncut lattice tet), float64 from the stored positions: smallest, median, and the
                share of children below 1e-3 and below 1e-6.  Slivers are expected: a cut arbitrarily close to a lattice vertex gives an
                arbitrarily thin child, and nothing is snapped.
Timing: host clock round a device synchronisation, 5 calls, median (min - max).  Records, not gates: no test asserts any of them, and nothing in the
repository claims a speed from them."""
import argparse
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'd3human-code_amd')
sys.path.insert(0, PKG)
from d3h import meshops, mtets, tetfill, watertight          # noqa: E402


def uv_sphere(n_lat=100, n_lon=100, r=0.5):
    th = np.linspace(0, np.pi, n_lat + 1)[1:-1]
    ph = np.arange(n_lon) * (2 * np.pi / n_lon)
    ring = np.stack([np.outer(np.sin(th), np.cos(ph)), np.outer(np.sin(th), np.sin(ph)), np.outer(np.cos(th), np.ones(n_lon))], -1).reshape(-1, 3)
    v = np.concatenate([[[0, 0, 1.0]], ring, [[0, 0, -1.0]]]) * r
    idx = lambda i, j: 1 + i * n_lon + j % n_lon
    f = [(0, idx(0, j), idx(0, j + 1)) for j in range(n_lon)]
    for i in range(n_lat - 2):
        for j in range(n_lon):
            f += [(idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)), (idx(i, j), idx(i + 1, j + 1), idx(i, j + 1))]
    last = len(v) - 1
    f += [(last, idx(n_lat - 2, j + 1), idx(n_lat - 2, j)) for j in range(n_lon)]
    return v.astype(np.float32), np.array(f, np.int64)


def timed(fn, reps=5):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def main(dev='cuda'):
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'tetfill_probe.md'))
    ap.add_argument('--commit', default=None)
    ap.add_argument('--res', type=int, nargs='+', default=[64, 128])
    a = ap.parse_args()
    commit = a.commit
    if commit is None:
        try:
            commit = subprocess.check_output(['git', '-C', ROOT, 'rev-parse', '--short', 'HEAD'], stderr=subprocess.DEVNULL).decode().strip()
        except Exception:
            commit = 'unknown'
    v_np, f_np = uv_sphere()
    mv, mf = torch.from_numpy(v_np).to(dev), torch.from_numpy(f_np).to(dev)
    meshops.mesh_wsdf(mv[:8].contiguous(), mv, mf, want_w=False)          # the library is loaded, the kernels' code objects are resident
    lines = [f'# Tet fill probe ({commit}; {torch.cuda.get_device_name(0)})', '',
             f'fill_mesh on a closed sphere of {len(f_np)} faces, scale 1.1.  Times in milliseconds, host clock round a device synchronisation: median '
             '(min - max) of 5 calls; the first call once.  Records, not gates.', '']
    for res in a.res:
        watertight._lattices.clear()
        mtets.TetGrid._cache.clear()
        first = timed(lambda: tetfill.fill_mesh(mv, mf, res=res), reps=1)[0]
        v, t, h = tetfill.fill_mesh(mv, mf, res=res)
        unit, tets = watertight._lattice(res, mv.device)
        lo, hi = mv.min(0).values, mv.max(0).values
        pos = ((lo + hi) * 0.5 + unit * (float((hi - lo).max()) * 1.1 * 0.5)).contiguous()
        sdf, _ = meshops.mesh_wsdf(pos, mv, mf, want_w=False)
        n_in = int((~(sdf > 0)).sum())
        p = v.double()[t]
        vol = (torch.linalg.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]) * (p[:, 3] - p[:, 0])).sum(-1) / 6.0
        rel = (vol / (h ** 3 / 6.0)).cpu().numpy()
        lines += [f'## res {res}: {pos.shape[0]} lattice vertices, {tets.shape[0]} tets, pitch {h:.6f}', '',
                  f'{n_in} inside vertices + {v.shape[0] - n_in} cut vertices = {v.shape[0]} vertices; {t.shape[0]} children; summed volume {float(vol.sum()):.6f} '
                  f'(the sphere: {4 / 3 * np.pi * 0.125:.6f})', '',
                  f'child volume / (h^3 / 6): smallest {rel.min():.3e}, median {np.median(rel):.3e}; below 1e-3: {100.0 * (rel < 1e-3).mean():.2f} %, below 1e-6: '
                  f'{100.0 * (rel < 1e-6).mean():.3f} %, negative: {int((rel < 0).sum())}', '',
                  '| what | median ms | min | max |', '|---|---|---|---|', f'| fill_mesh, first call (lattice + edge tables built) | {first:.1f} | | |']
        for what, fn in (('fill_mesh, later calls', lambda: tetfill.fill_mesh(mv, mf, res=res)),
                         ('meshops.mesh_wsdf on the lattice vertices', lambda: meshops.mesh_wsdf(pos, mv, mf, want_w=False)),
                         ('tetfill.clip', lambda: tetfill.clip(pos, sdf, tets))):
            m = timed(fn)
            lines.append(f'| {what} | {m[0]:.2f} | {m[1]:.2f} | {m[2]:.2f} |')
            print(lines[-1], flush=True)
        lines.append('')
        del p, vol, v, t, pos, sdf
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')
    print('wrote', a.out)


if __name__ == '__main__':
    main()
