"""Probe of the distance queries on the BVH (csrc/bvhdist.hip) beside the brute-force mesh_wsdf, at the sizes of profiles/handoff_probe.md: time of the
brute-force query, of the BVH build, of the node moments and of the query at beta 2, 3 and 4; the error of the hierarchical winding number against a
float64 sum over all triangles on a 4096-query sample; the number of signs that differ from the brute-force route.  Writes profiles/bvhdist_probe.md.
Nothing is asserted: the defaults stay brute force, and a later change may move them on this file's evidence.

    python tools/gpu_probe_bvhdist.py [--out profiles/bvhdist_probe.md] [--small]

The meshes are the synthetic stand-ins of tools/gpu_probe_handoff.py, through the same steps: the merged open body (37 000 faces), the refined garment
(49 280 faces) with the 11 400 vertices of the SMPL part under it as push queries, and the closed capsule of 21 000 faces for SMPL-X (20 908 faces).
--small shrinks every query set (a rehearsal of the script, not a measurement)."""
import argparse
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'd3human-code_amd'), os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')]
BETAS = (2.0, 3.0, 4.0)
REPS = 3


def winding64(q, v, f, chunk=128):
    """w in turns, float64 on the queries' device: van Oosterom-Strackee summed over all triangles"""
    t = v.double()[f.long()]
    A, B, C = t[None, :, 0], t[None, :, 1], t[None, :, 2]
    out = []
    for s in range(0, q.shape[0], chunk):
        p = q[s:s + chunk].double()[:, None]
        ra, rb, rc = A - p, B - p, C - p
        la, lb, lc = ra.norm(dim=-1), rb.norm(dim=-1), rc.norm(dim=-1)
        det = (ra * torch.cross(rb, rc, dim=-1)).sum(-1)
        den = la * lb * lc + (ra * rb).sum(-1) * lc + (ra * rc).sum(-1) * lb + (rb * rc).sum(-1) * la
        out.append((2.0 * torch.atan2(det, den)).sum(1) / (4.0 * math.pi))
    return torch.cat(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'bvhdist_probe.md'))
    ap.add_argument('--small', action='store_true')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('gpu_probe_bvhdist: no GPU -- a time taken anywhere else says nothing')
    import handoff_cases as HC
    from gpu_probe_handoff import capsule
    from d3h import meshops as MO, meshrefine as MR, meshtopo as MT, raytrace as RT
    dev = 'cuda'
    T = lambda x, dt=None: torch.as_tensor(np.ascontiguousarray(x), dtype=dt, device=dev)

    def timed(fn):
        """-> (median ms of REPS runs after one warm-up, the last result)"""
        fn()
        ms = []
        for _ in range(REPS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ms), out

    # the meshes, by the steps of tools/gpu_probe_handoff.py (the push moves nothing there and is left out)
    v, f, zm = capsule(100, 56)
    gv, gf = HC.cylinder(radius=0.28, height=0.8, nu=160, nz=60)
    cloth_v, cloth_f, _ = MR.refine_long_edges(T(gv, torch.float32), T(gf), 4 / 3 * 0.01, 3)
    cv, cf = HC._compact(v, f[np.abs(zm) < 0.3])
    cut_v, cut_f, _ = MR.refine_long_edges(T(cv, torch.float32), T(cf), 4 / 3 * 0.01, 3)
    cut_f = MT.peel_open_faces(cut_f, cut_v.shape[0], 1)
    bv, bf = HC._compact(v, f[np.abs(zm) > 0.26])
    body_f = MT.peel_open_faces(T(bf), len(bv), 2)
    mv, mf = MT.merge_and_repair(cut_v.double(), cut_f.long(), T(bv), body_f.long())
    mv, mf = mv.float().contiguous(), mf.int().contiguous()
    sv, sf = T(v, torch.float32), T(f).int().contiguous()

    def lattice(n, mesh_v, scale=1.1):
        lo, hi = mesh_v.min(0).values, mesh_v.max(0).values
        g = torch.linspace(-0.5, 0.5, n, device=dev)
        return ((lo + hi) * 0.5 + torch.stack(torch.meshgrid(g, g, g, indexing='ij'), -1).reshape(-1, 3) * float((hi - lo).max()) * scale).contiguous()

    shrink = 8 if a.small else 1
    cases = [('merged open body against the 128^3 lattice vertices', mv, mf, lattice(129 // shrink, mv)),
             ('merged open body against the 256^3 lattice vertices', mv, mf, lattice(257 // shrink, mv)),
             ('garment against the push queries, one round', cloth_v.float().contiguous(), cloth_f.int().contiguous(), cut_v.float().contiguous()[::shrink]),
             ('closed SMPL-X stand-in against a 64^3 grid', sv, sf, lattice(64 // shrink, sv))]
    out = ['# Distance queries on the BVH beside the brute-force mesh_wsdf: probe at the real sizes\n',
           'Written by tools/gpu_probe_bvhdist.py on an MI355X (' + torch.cuda.get_device_name(0) + '). Every time is the median of ' + str(REPS) +
           ' runs after one warm-up run of the same shape, host clock around the call with a device synchronisation on both sides (so the launches\' '
           'host side is inside). Both routes give the signed distance only (`want_w=False`), as the pipeline asks for it. `w64` is the float64 '
           'van Oosterom-Strackee sum over all triangles on a seeded sample of 4096 of the queries. Nothing is asserted on these numbers; the defaults '
           'stay brute force.\n' + ('\n**--small: every query set is shrunk; a rehearsal, not a measurement.**\n' if a.small else '')]
    for name, cv_, cf_, q in cases:
        F, n = int(cf_.shape[0]), int(q.shape[0])
        t_brute, (s_brute, _) = timed(lambda: MO.mesh_wsdf(q, cv_, cf_, want_w=False, check=False))
        t_build, bvh = timed(lambda: RT.Bvh(cv_, cf_))

        def moments():
            bvh.moments = None
            bvh.winding(q[:1])
        t_mom, _ = timed(moments)                                            # includes one one-query launch
        t_near, near = timed(lambda: bvh.nearest(q))
        sel = torch.randperm(n, generator=torch.Generator().manual_seed(0))[:4096].to(dev)
        w64 = winding64(q[sel], cv_, cf_)
        mag = int((s_brute.abs().cpu().numpy().view(np.uint32) != np.sqrt(near.d2.cpu().numpy()).view(np.uint32)).sum())      # numpy's root: correctly rounded
        out.append(f'\n## {name}\n\n{F} faces, {n} queries. Brute force: **{t_brute:.1f} ms**. BVH build {t_build:.2f} ms, node moments {t_mom:.2f} ms, '
                   f'nearest triangle alone (d2, tri, bary) {t_near:.2f} ms; {mag} of {n} magnitudes differ in their bits from the brute-force route'
                   f'.\n\n'
                   '| beta | signed_distance, ms | build + moments + query, ms | speed-up over brute force | max abs(w - w64) | mean abs(w - w64) | signs that differ from brute force |\n'
                   '|---:|---:|---:|---:|---:|---:|---:|\n')
        for beta in BETAS:
            t_q, s = timed(lambda: bvh.signed_distance(q, beta=beta))
            w = bvh.winding(q[sel], beta=beta).double()
            err = (w - w64).abs()
            diff = int((torch.signbit(s) != torch.signbit(s_brute)).sum())
            tot = t_build + t_mom + t_q
            out.append(f'| {beta:g} | {t_q:.2f} | {tot:.2f} | {t_brute / tot:.1f} x | {float(err.max()):.2e} | {float(err.mean()):.2e} | {diff} of {n} |\n')
        del bvh, near, s_brute
    with open(a.out, 'w') as fp:
        fp.write(''.join(out))
    print(open(a.out).read())


if __name__ == '__main__':
    main()
