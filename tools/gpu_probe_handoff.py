"""Probe of the second half of the stage hand-off at its real sizes (script/process_body_cloth_head_msdfcut.py of this build): time and peak device
memory of each step, the share of the collision push, the cap residual after the relaxation.  Writes profiles/handoff_probe.md.  Nothing is asserted.

    python tools/gpu_probe_handoff.py [--out profiles/handoff_probe.md]

The inputs are synthetic stand-ins of the real sizes: a capsule of 20 908-odd faces for SMPL-X (20 908 faces), an open cylindrical shell 0.03 outside its
middle as the garment (19 200 faces before refinement; the split stage's garment is of that order), the capsule's ends as the visible body parts."""
import argparse
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'd3human-code_amd'), os.path.join(ROOT, 'tests')]


def capsule(nu, nz):
    r, half = 0.25, 0.6
    cap = [t for t in np.linspace(0, np.pi / 2, nu // 4 + 1)[1:-1]]
    zs = [-half - r * math.cos(t) for t in cap] + list(np.linspace(-half, half, nz + 1)) + [half + r * math.sin(t) for t in cap]
    rad = lambda z: r if abs(z) <= half else math.sqrt(max(r * r - (abs(z) - half) ** 2, 0.0))
    ang = 2 * np.pi * np.arange(nu) / nu
    v = np.concatenate([[[0, 0, -half - r]]] + [np.stack([rad(z) * np.cos(ang), rad(z) * np.sin(ang), np.full(nu, z)], 1) for z in zs] + [[[0, 0, half + r]]])
    i = np.arange(nu)
    f = [np.stack([np.zeros(nu, np.int64), 1 + (i + 1) % nu, 1 + i], 1)]
    for k in range(len(zs) - 1):
        a, b = 1 + k * nu + i, 1 + k * nu + (i + 1) % nu
        f += [np.stack([a, b, b + nu], 1), np.stack([a, b + nu, a + nu], 1)]
    base = 1 + (len(zs) - 1) * nu
    f.append(np.stack([base + i, base + (i + 1) % nu, np.full(nu, len(v) - 1)], 1))
    f = np.concatenate(f)
    return v, f, v[f][:, :, 2].mean(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'handoff_probe.md'))
    a = ap.parse_args()
    import handoff_cases as HC
    from d3h import imgops as IO, meshops as MO, meshrefine as MR, meshtopo as MT, watertight as WT
    dev = 'cuda'
    T = lambda x, dt=None: torch.as_tensor(np.ascontiguousarray(x), dtype=dt, device=dev)
    rows, lines = [], []

    def step(name, fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        rows.append((name, (time.perf_counter() - t0) * 1e3, torch.cuda.max_memory_allocated() / 2 ** 20))
        return out

    v, f, zm = capsule(100, 56)
    gv, gf = HC.cylinder(radius=0.28, height=0.8, nu=160, nz=60)
    lines.append(f'SMPL stand-in: {len(f)} faces; garment: {len(gf)} faces; covered middle |z| < 0.3, visible parts |z| > 0.26; target_len 0.01')
    step('warm-up (library load, first launches)', lambda: MR.refine_long_edges(T(gv, torch.float32), T(gf), 1.0))
    cloth_v, cloth_f, _ = step('refine garment (3 rounds, 0.0133)', lambda: MR.refine_long_edges(T(gv, torch.float32), T(gf), 4 / 3 * 0.01, 3))
    cv, cf = HC._compact(v, f[np.abs(zm) < 0.3])
    cut_v, cut_f, _ = step('refine covered SMPL (3 rounds)', lambda: MR.refine_long_edges(T(cv, torch.float32), T(cf), 4 / 3 * 0.01, 3))
    cut_f = step('peel one ring', lambda: MT.peel_open_faces(cut_f, cut_v.shape[0], 1))
    nrm = step('vertex normals', lambda: IO.auto_normals(cut_v, cut_f.int()))
    cf32 = cloth_f.int().contiguous()
    field = lambda x: -MO.mesh_wsdf(x, cloth_v, cf32, want_w=False)[0]
    # the stand-in body is 0.03 inside the garment and needs no push: every round is forced so that the cost of 100 rounds is on record
    t_one = step('push: one round (field + push)', lambda: MO.collision_push(cut_v, nrm, field, rounds=1))
    pushed, pushes = step('push: 100 rounds, none stopping early', lambda: MO.collision_push(cut_v, nrm, field, rounds=100, stop_when_still=False))
    lines.append(f'refined garment: {cloth_f.shape[0]} faces; pushed SMPL part: {cut_v.shape[0]} vertices, {int((pushes > 0).sum())} of them moved')
    bv, bf = HC._compact(v, f[np.abs(zm) > 0.26])
    body_f = step('peel two rings off the body parts', lambda: MT.peel_open_faces(T(bf), len(bv), 2))
    mv, mf = step('merge and weld', lambda: MT.merge_and_repair(pushed.double(), cut_f.long(), T(bv), body_f.long()))
    mv = mv.float()
    lines.append(f'merged open body: {mv.shape[0]} vertices, {mf.shape[0]} faces')
    for res in (128, 256):
        try:
            if res == 256:
                # the lattice tables of 256^3 cells (100 M tets, 8 x those of 128) are not built here: the field query alone, on the lattice vertices
                g = torch.linspace(-0.5, 0.5, res + 1, device=dev)
                pos = torch.stack(torch.meshgrid(g, g, g, indexing='ij'), -1).reshape(-1, 3) * 1.1 * 1.7
                step(f'watertight res {res}: mesh_wsdf on {pos.shape[0]} lattice vertices only', lambda: MO.mesh_wsdf(pos, mv, mf, want_w=False))
                lines.append('res 256: only the field query was run; the Kuhn lattice of 256^3 cells (100 M tets and their edge tables, built on the host by '
                             'synth.kuhn_grid and mtets.TetGrid) was not built, so extraction and relaxation at 256 are not measured')
                continue
            step(f'watertight res {res}: lattice tables (once per resolution)', lambda: WT._lattice(res, dev))
            wv0, wf, cap, h = step(f'watertight res {res}: field, marching tets, cap query', lambda: WT.extract(mv, mf, res=res))
            wv = step(f'watertight res {res}: relax 32 rounds', lambda: MR.relax(wv0, wf, cap, 32))
            rv, rf, _ = step(f'refine the watertight body (3 rounds)', lambda: MR.refine_long_edges(wv, wf, 4 / 3 * 0.01, 3))
            # cap residual: distance of the cap vertices to the capsule they bridge (radius 0.25 round the axis, on the cylinder part), in cells
            c0, c1 = wv0[cap].double().cpu().numpy(), wv[cap].double().cpu().numpy()
            res0, res1 = np.abs(np.hypot(c0[:, 0], c0[:, 1]) - 0.25), np.abs(np.hypot(c1[:, 0], c1[:, 1]) - 0.25)
            lines.append(f'res {res}: h = {h:.5f}; {wv.shape[0]} vertices, {wf.shape[0]} faces, {int(cap.sum())} cap vertices; cap residual (distance to the '
                         f'capsule surface) before the relaxation max {res0.max() / h:.3f} h rms {np.sqrt((res0 ** 2).mean()) / h:.3f} h, after max '
                         f'{res1.max() / h:.3f} h rms {np.sqrt((res1 ** 2).mean()) / h:.3f} h; refined: {rf.shape[0]} faces')
            far = torch.as_tensor(np.abs(v[:, 2]) < 0.2, device=dev) | torch.as_tensor(np.abs(v[:, 2]) > 0.4, device=dev)
            d = torch.cdist(T(v, torch.float32)[far][::25], wv).min(1).values.max()
            lines.append(f'res {res}: input vertices away from the cuts -> nearest result vertex: max {float(d) / h:.3f} h (the tests bound it by 2 h)')
        except Exception as e:                                                 # a probe: record and go on
            lines.append(f'res {res}: failed with {type(e).__name__}: {e}')
    total = sum(r[1] for r in rows[1:] if 'one round' not in r[0] and '256' not in r[0])
    push = [r[1] for r in rows if r[0].startswith('push: 100')][0]
    with open(a.out, 'w') as fp:
        fp.write('# Stage hand-off, second half: probe at the real sizes\n\nWritten by tools/gpu_probe_handoff.py on an MI355X (' +
                 torch.cuda.get_device_name(0) + '). One run, host wall-clock around each step with a device synchronisation on both sides; the first '
                 'row absorbs the library load. Nothing is asserted on these numbers.\n\n')
        fp.write('\n'.join('- ' + ln for ln in lines) + '\n\n| step | ms | peak device memory, MiB |\n|---|---:|---:|\n')
        fp.write('\n'.join(f'| {n} | {ms:.1f} | {mb:.0f} |' for n, ms, mb in rows) + '\n\n')
        fp.write(f'Sum of the steps of one hand-off at res 128 (the forced 100 push rounds included): {total:.0f} ms; the 100 push rounds take {push:.0f} ms = '
                 f'{100 * push / total:.0f} % of it. In a real hand-off the push stops at the first round that moves nothing.\n')
        if push > 0.5 * total:
            fp.write('\nThe push dominates: its queries are few (one thread each) against many triangles. Follow-up, not built here: a second grid dimension '
                     'of mesh_wsdf that splits the triangles, with a combine pass.\n')
    print(open(a.out).read())


if __name__ == '__main__':
    main()
