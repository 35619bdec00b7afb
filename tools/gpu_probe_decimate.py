"""Probe of quadric decimation (d3h.meshrefine.decimate, csrc/meshdecim.hip) at the export's real sizes, on the garment and the watertight body of
tools/gpu_probe_remesh.py, each reduced to 1/4 and to 1/16 of its faces: time in total and per round, rounds used, faces reached, the largest cost taken
and the RMS distance to the input both ways -- beside collapse_short_edges driven to the same counts.  It also writes the figures the tests assert
(tests/decimate_cases.py: the lumpy sphere against the classic one-at-a-time algorithm, the cube).  Writes profiles/decimate_probe.md.  Nothing is
asserted; no default depends on it.

    python tools/gpu_probe_decimate.py [--out profiles/decimate_probe.md]

The rounds of decimate are walked here from the same internal functions with a device synchronisation around each, and the result is checked to be the
public function's, bit for bit."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'd3human-code_amd'), os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'decimate_probe.md'))
    a = ap.parse_args()
    import handoff_cases as HC
    import gpu_probe_handoff as PH
    from d3h import meshrefine as MR, meshtopo as MT, raytrace as RT, watertight as WT
    dev = 'cuda'
    T = lambda x, dt=None: torch.as_tensor(np.ascontiguousarray(x), dtype=dt, device=dev)
    out = []

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return r, (time.perf_counter() - t0) * 1e3

    def rms(v, f, v0, f0, bvh0):
        """RMS distance result vertices -> input surface, input vertices -> result surface"""
        fwd = bvh0.nearest(v[torch.unique(f.long())].contiguous()).d2.double().mean().sqrt()
        back = RT.Bvh(v, f).nearest(v0[torch.unique(f0.long())].contiguous()).d2.double().mean().sqrt()
        return f'{float(fwd):.3e} / {float(back):.3e}'

    def walk(v, f, target):
        """decimate(v, f, target) round by round -> (v', f', ms per round, largest cost)"""
        Q, _ = MR._quadrics(v, f, True)
        ms, worst = [], 0.0
        for rnd in range(256):
            if f.shape[0] <= target:
                break
            r, t = clock(lambda: MR._decimate_round(v, f, Q, None, target, 3.0, 256, True, float('inf'), rnd))
            if r is None:
                break
            ms.append(t)
            v, f, Q, worst = r[0], r[1], r[5], max(worst, r[7])
        return v, f, ms, worst

    def short_route(v, f, target):
        """collapse_short_edges one round at a time, lo = the length below which just enough edges lie (a device sort per round, inside the time)"""
        rounds = 0
        for _ in range(1000):
            nf = int(f.shape[0])
            if nf <= target:
                break
            fl = f.long()
            e = torch.unique(torch.sort(torch.cat([fl[:, [0, 1]], fl[:, [1, 2]], fl[:, [2, 0]]]), 1).values, dim=0)
            L = torch.sort((v[e[:, 0]] - v[e[:, 1]]).norm(dim=1)).values
            lo = float(L[min((nf - target + 1) // 2, L.numel() - 1)]) * (1 + 1e-6)
            nv, nf_, _, _ = MR.collapse_short_edges(v, f, lo, 1e9, rounds=1)
            if nf_.shape[0] == nf:
                break
            v, f, rounds = nv, nf_, rounds + 1
        return v, f, rounds

    def probe(name, v0, f0):
        out.append(f'\n## {name}\n')
        out.append('| target | route | faces reached | rounds | ms in total | ms per round: median (min .. max) | largest cost | RMS to the input / from the input |\n'
                   '|---:|---|---:|---:|---:|---:|---:|---|')
        bvh0 = RT.Bvh(v0, f0)
        F = int(f0.shape[0])
        for div in (4, 16):
            target = F // div
            (gv, gf, _, _, info), total = clock(lambda: MR.decimate(v0, f0, target))
            wv, wf, ms, worst = walk(v0, f0, target)
            same = torch.equal(wv, gv) and torch.equal(wf, gf) and worst == info['max_cost'] and len(ms) == info['rounds']
            out.append(f"| {target} (1/{div}) | decimate | {gf.shape[0]} | {info['rounds']} | {total:.1f} | {np.median(ms):.2f} ({min(ms):.2f} .. {max(ms):.2f}) | "
                       f"{info['max_cost']:.3e} | {rms(gv, gf, v0, f0, bvh0)} |" + ('' if same else ' (the walk differs from the public call!)'))
            (sv, sf, rounds), total = clock(lambda: short_route(v0, f0, target))
            out.append(f'| {target} (1/{div}) | collapse_short_edges | {sf.shape[0]} | {rounds} | {total:.1f} | {total / max(rounds, 1):.2f} (mean) | | {rms(sv, sf, v0, f0, bvh0)} |')

    MR.decimate(T(HC.cylinder()[0], torch.float32), T(HC.cylinder()[1]), 8)                     # library load, first launches
    gv, gf = HC.cylinder(radius=0.28, height=0.8, nu=160, nz=60)
    probe(f'Garment stand-in (open cylinder, {len(gf)} faces)', T(gv, torch.float32), T(gf))
    v, f, zm = PH.capsule(100, 56)
    t = 0.01
    cv, cf = HC._compact(v, f[np.abs(zm) < 0.3])
    cut_v, cut_f, _ = MR.refine_long_edges(T(cv, torch.float32), T(cf), t * 4.0 / 3.0, 3)
    cut_f = MT.peel_open_faces(cut_f, cut_v.shape[0], 1)
    bv, bf = HC._compact(v, f[np.abs(zm) > 0.26])
    body_f = MT.peel_open_faces(T(bf), len(bv), 2)
    mv, mf = MT.merge_and_repair(cut_v.double(), cut_f.long(), T(bv), body_f.long())
    wv, wf, _ = WT.watertight(mv.float(), mf, res=128, relax_iters=32)
    probe(f'Watertight body (res 128, {wf.shape[0]} faces)', wv.contiguous(), wf.contiguous())
    # the figures the tests assert (tests/decimate_cases.py)
    import decimate_cases as DC
    out.append('\n## The test cases\n')
    v, f = DC.lumpy_sphere()
    for target in (320, 128):
        gv, gf, _, _, info = DC.run(dev, v, f, target)
        rv, rf, ref = DC.quality_reference()[target]
        got = DC.rms_pair(v, f, gv, gf)
        sv, sf = DC._short_edge_route(dev, v, f, target)
        short = DC.rms_pair(v, f, sv, sf)
        out.append(f"- lumpy sphere 1280 -> {target}: {len(gf)} faces in {info['rounds']} rounds, largest cost {info['max_cost']:.3e}; RMS to the input / from the input: "
                   f'rounds {got[0]:.5f} / {got[1]:.5f}, classic one-at-a-time {ref[0]:.5f} / {ref[1]:.5f} (ratio {got[0] / ref[0]:.3f} / {got[1] / ref[1]:.3f}, bound 1.25), '
                   f'collapse_short_edges at {len(sf)} faces {short[0]:.5f} / {short[1]:.5f} (ratio {got[0] / short[0]:.3f} / {got[1] / short[1]:.3f}, bound 0.5)')
    for k, target in ((4, 24), (8, 48)):
        v, f = DC.cube(k)
        gv, gf, _, _, info = DC.run(dev, v, f, target)
        out.append(f"- cube, {k} x {k} quads per side, {len(f)} -> {target}: {len(gf)} faces in {info['rounds']} rounds, largest cost {info['max_cost']:.3e}, volume "
                   f'{float(DC.volume(gv, gf))!r}')
    v, f = DC.ico(2)
    info = DC.run(dev, v, f, 80)[4]
    out.append(f"- icosphere(2) 320 -> 80: {info['rounds']} rounds, {info['collapses']} collapses")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fp:
        fp.write('# Quadric decimation for the level-of-detail export\n\nWritten by tools/gpu_probe_decimate.py on an MI355X (' + torch.cuda.get_device_name(0) +
                 '). Defaults throughout (rounds = 256, window = 3.0, min_window = 256, boundary = \'slide\'). Host wall-clock with a device synchronisation on both '
                 'sides; "ms in total" is one call of the public function, "ms per round" the same rounds walked one at a time. Every round rebuilds its adjacency '
                 'with torch sorts and reads its counters back once; that time is inside the round. RMS distances are over the vertices of one mesh to the '
                 'surface of the other (Bvh.nearest). Nothing is asserted on these numbers and no default depends on them.\n')
        fp.write('\n'.join(out) + '\n')
    print(open(a.out).read())


if __name__ == '__main__':
    main()
