"""Probe of the two remeshing routes of the stage hand-off (process_body_msdf_distance_bodyedge(remesh='split' | 'isotropic')) at its real sizes, on the
garment and the watertight body of tools/gpu_probe_handoff.py: time per step and per round, rounds used, collapses and flips per round, edge lengths,
minimum angle, valences and the Hausdorff distance to the input.  Writes profiles/remesh_probe.md.  Nothing is asserted; no default depends on it.

    python tools/gpu_probe_remesh.py [--out profiles/remesh_probe.md] [--repeat 5]

Every step is a pure function of its inputs, so each is called `--repeat` times on the same tensors: the median is reported, with the smallest and the
largest call.  The loop of d3h.meshrefine.isotropic_remesh is walked here step by step from the same internal functions, and its result is checked to
be the public function's, bit for bit."""
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
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'remesh_probe.md'))
    ap.add_argument('--repeat', type=int, default=5)
    a = ap.parse_args()
    import handoff_cases as HC
    import gpu_probe_handoff as PH
    from d3h import meshrefine as MR, meshtopo as MT, raytrace as RT, watertight as WT
    dev = 'cuda'
    T = lambda x, dt=None: torch.as_tensor(np.ascontiguousarray(x), dtype=dt, device=dev)
    t = 0.01
    hi, lo = t * 4.0 / 3.0, t * 4.0 / 5.0
    out = []

    def timed(fn):
        ms = []
        for _ in range(a.repeat):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        return r, float(np.median(ms)), min(ms), max(ms)

    def fmt(m):
        return f'{m[1]:.2f} ({m[2]:.2f} .. {m[3]:.2f})'

    def quality(v, f, bvh0, v0, f0):
        v64, fl = v.double(), f.long()
        e = torch.unique(torch.sort(torch.cat([fl[:, [0, 1]], fl[:, [1, 2]], fl[:, [2, 0]]]), 1).values, dim=0)
        L = (v64[e[:, 0]] - v64[e[:, 1]]).norm(dim=1)
        p = v64[fl]
        ang = []
        for k in range(3):
            u, w = p[:, (k + 1) % 3] - p[:, k], p[:, (k + 2) % 3] - p[:, k]
            ang.append(torch.acos(((u * w).sum(1) / (u.norm(dim=1) * w.norm(dim=1)).clamp_min(1e-300)).clamp(-1, 1)))
        ang = torch.rad2deg(torch.stack(ang, 1))
        val = torch.bincount(e.reshape(-1))
        val = val[val > 0]
        hist = torch.bincount(val.clamp(max=9), minlength=10).tolist()
        fwd = bvh0.nearest(v[torch.unique(fl)]).d2.max().sqrt()
        back = RT.Bvh(v, f).nearest(v0[torch.unique(f0.long())]).d2.max().sqrt()
        return (f'{v.shape[0]} vertices, {f.shape[0]} faces; edges: {100 * float((L < lo).double().mean()):.1f} % below 4/5 t, {100 * float((L > hi).double().mean()):.1f} % above 4/3 t, '
                f'min {float(L.min()) / t:.3f} t, max {float(L.max()) / t:.3f} t; min angle {float(ang.min()):.2f} deg, {100 * float((ang.min(1).values < 20).double().mean()):.1f} % of faces '
                f'below 20 deg; valence 3..9+: {hist[3:]} ({100 * hist[6] / max(sum(hist), 1):.1f} % valence 6); Hausdorff result -> input {float(fwd) / t:.4f} t, input -> result '
                f'{float(back) / t:.4f} t')

    def probe(name, v0, f0):
        out.append(f'\n## {name}\n')
        bvh0 = RT.Bvh(v0, f0)
        out.append(f'- input: {quality(v0, f0, bvh0, v0, f0)}')
        (sv, sf, _), *m = timed(lambda: MR.refine_long_edges(v0, f0, hi, 3))
        out.append(f"- `'split'` (refine_long_edges, 3 rounds): {fmt((None, *m))} ms; {quality(sv, sf, bvh0, v0, f0)}")
        (iv, if_, _), *m = timed(lambda: MR.isotropic_remesh(v0, f0, t, 3))
        out.append(f"- `'isotropic'` (isotropic_remesh, 3 iterations, its own BVH build included): {fmt((None, *m))} ms; {quality(iv, if_, bvh0, v0, f0)}")
        (_, *m) = timed(lambda: RT.Bvh(v0, f0))
        out.append(f'- the BVH of the input alone: {fmt((None, *m))} ms')
        out.append('\n| iteration | step | ms: median (min .. max) | what it did |\n|---|---|---:|---|')
        v, f, f0l = v0, f0, f0.long()
        for it in range(3):
            n = v.shape[0]
            r = timed(lambda: MR.refine_long_edges(v, f, hi, iterations=1))
            out.append(f'| {it + 1} | split | {fmt(r)} | {r[0][0].shape[0] - n} edges split |')
            v, f = r[0][0], r[0][1]
            moved = torch.zeros(v.shape[0], dtype=torch.bool, device=dev)
            moved[n:] = True
            before, src = v, torch.arange(v.shape[0], device=dev)
            carried = moved
            for k in range(8):
                r = timed(lambda: MR._collapse_round(v, f, lo, hi, None))
                if r[0] is None:
                    out.append(f'| {it + 1} | collapse round {k + 1} | {fmt(r)} | nothing: the loop ends |')
                    break
                out.append(f'| {it + 1} | collapse round {k + 1} | {fmt(r)} | {v.shape[0] - r[0][0].shape[0]} collapses |')
                nv, f, _, vm, keep = r[0]
                carried = torch.zeros(nv.shape[0], dtype=torch.long, device=dev).index_add_(0, vm, carried.long()) > 0
                v, src = nv, src[keep]
            moved = carried | (v != before[src]).any(1)
            for k in range(8):
                r = timed(lambda: MR._flip(v, f, 1, None))
                out.append(f'| {it + 1} | flip round {k + 1} | {fmt(r)} | {r[0][1]} flips |')
                f = r[0][0]
                if r[0][1] == 0:
                    break
            r = timed(lambda: MR._smooth(v, f, None))
            moved |= (r[0] != v).any(1)
            out.append(f'| {it + 1} | smooth | {fmt(r)} | {int((r[0] != v).any(1).sum())} of {v.shape[0]} vertices moved |')
            v = r[0]
            at = torch.nonzero(moved).reshape(-1)
            r = timed(lambda: MR._reproject(v, at, bvh0, v0, f0l))
            out.append(f'| {it + 1} | reproject | {fmt(r)} | {at.numel()} vertices |')
            v = r[0]
        same = torch.equal(v, iv) and torch.equal(f, if_)
        out.append(f'\nThe walk above ends in the result of `isotropic_remesh`, bit for bit: {same}.')

    MR.refine_long_edges(T(HC.cylinder()[0], torch.float32), T(HC.cylinder()[1]), 1.0)          # library load, first launches
    gv, gf = HC.cylinder(radius=0.28, height=0.8, nu=160, nz=60)
    probe(f'Garment stand-in (open cylinder, {len(gf)} faces)', T(gv, torch.float32), T(gf))
    v, f, zm = PH.capsule(100, 56)
    cv, cf = HC._compact(v, f[np.abs(zm) < 0.3])
    cut_v, cut_f, _ = MR.refine_long_edges(T(cv, torch.float32), T(cf), hi, 3)
    cut_f = MT.peel_open_faces(cut_f, cut_v.shape[0], 1)
    bv, bf = HC._compact(v, f[np.abs(zm) > 0.26])
    body_f = MT.peel_open_faces(T(bf), len(bv), 2)
    mv, mf = MT.merge_and_repair(cut_v.double(), cut_f.long(), T(bv), body_f.long())
    wv, wf, _ = WT.watertight(mv.float(), mf, res=128, relax_iters=32)
    probe(f'Watertight body (res 128, {wf.shape[0]} faces)', wv.contiguous(), wf.contiguous())
    # the figures the tests assert (tests/remesh_cases.py): the sequential restatement and this build on the jittered icosphere(3)
    import remesh_cases as RC
    out.append('\n## The test case: icosphere(3), 1280 faces, radius 0.8, tangential jitter 0.02\n')
    for open_cap, tt in ((False, 0.12), (True, 0.2)):
        sv, sf = RC.sphere_case(open_cap)
        (yv, yf, _), log = RC.isotropic_reference(open_cap)
        gv, gf, _ = MR.isotropic_remesh(T(sv), T(sf), tt, 3)
        out.append(f"- {'open (cap z > 0.6 removed)' if open_cap else 'closed'}, t = {tt}, 3 iterations: input {RC.figures(sv, sf, tt)}; restatement {RC.figures(yv, yf, tt)}; this build "
                   f'{RC.figures(gv.cpu().numpy(), gf.cpu().numpy(), tt)}; Euler characteristic {HC._euler(sf)} -> {HC._euler(gf.cpu().numpy())}; open edges '
                   f'{int((HC._edges(sf)[1] == 1).sum())} -> {int((HC._edges(gf.cpu().numpy())[1] == 1).sum())}; restatement per iteration (vertices, faces, collapses per round, '
                   f'flips per round): {log}')
    out.append('\n(short / long: the share of edges below 4/5 t / above 4/3 t; val6: the share of valence-6 vertices.)')
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as fp:
        fp.write('# Remeshing at the hand-off: the split route against the isotropic route\n\nWritten by tools/gpu_probe_remesh.py on an MI355X (' +
                 torch.cuda.get_device_name(0) + f'). target_len t = {t}; host wall-clock around each call with a device synchronisation on both sides, median of '
                 f'{a.repeat} calls on the same inputs with the smallest and the largest in brackets. Nothing is asserted on these numbers and no default '
                 'depends on them. Every collapse and flip round rebuilds its adjacency with torch sorts; that time is inside the round.\n')
        fp.write('\n'.join(out) + '\n')
    print(open(a.out).read())


if __name__ == '__main__':
    main()
