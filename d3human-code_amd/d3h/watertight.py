"""Watertight extraction of an open, consistently wound triangle mesh: what the reference gets from meshlabserver with checkpoints/script/wt.mlx
(screened Poisson at depth 8, script/process_body_cloth_head_msdfcut.py:667,711).  Poisson reconstruction is not rebuilt; this is the project's own
route over pieces it already has:

    watertight(v, f, res=128, scale=1.1, relax_iters=32, accel='brute') -> (v', f', cap_mask)

  - a cube centred on the bounding box, side = scale x the longest extent (the scale of wt.mlx), filled with a synth.kuhn_grid(res, raw=True)
    lattice of pitch h = side / res
  - meshops.mesh_wsdf at the lattice vertices: the |w| = 0.5 surface of the winding number closes the holes
  - the watertight output of mtets.marching_tets, triangles wound outward
  - a vertex of the result is a CAP vertex when its distance to the input triangles exceeds h / 4 (a second mesh_wsdf query): across a cap the signed
    distance jumps from +d to -d, so linear interpolation puts cap vertices at edge midpoints, a staircase of amplitude at most h / 2
  - meshrefine.relax moves the cap vertices only (Jacobi, uniform Laplacian, everything else fixed): the staircase becomes a membrane.  The default
    of 32 rounds rests on gaps of at most about four cells and on a Jacobi sweep smoothing width k in about k^2 rounds.

res = 128 is the tet resolution the project trains at (Poisson depth 8 would correspond to 256).  cap_mask is bool [V'].
accel='bvh' answers both mesh_wsdf queries from one d3h.raytrace.Bvh of the input (meshops.mesh_wsdf, accel); the default is the brute-force loop."""
import torch

from . import meshops as _mo
from . import meshrefine as _mr
from . import mtets as _mtets
from . import synth as _synth

_lattices = {}


def _lattice(res, dev):
    key = (int(res), str(dev))
    if key not in _lattices:
        if len(_lattices) > 2:
            _lattices.clear()
        gv, gt = _synth.kuhn_grid(int(res), raw=True)
        _lattices[key] = (torch.as_tensor(gv, device=dev), torch.as_tensor(gt, device=dev))
    return _lattices[key]


def extract(v, f, res=128, scale=1.1, accel='brute'):
    """-> (v', f' int64, cap_mask, h): the closed surface before the relaxation"""
    v = v.detach().contiguous().float()
    if v.dim() != 2 or v.shape[1] != 3 or v.shape[0] == 0 or f.dim() != 2 or f.shape[1] != 3 or f.shape[0] == 0:
        raise RuntimeError(f'watertight: expected a mesh v [n,3], f [F,3] with n, F > 0, got {tuple(v.shape)} {tuple(f.shape)}')
    lo, hi = v.min(0).values, v.max(0).values
    side = float((hi - lo).max()) * float(scale)
    if not side > 0.0:
        raise RuntimeError('watertight: the mesh has no extent')
    unit, tets = _lattice(res, v.device)                                  # [-1, 1]^3
    pos = ((lo + hi) * 0.5 + unit * (side * 0.5)).contiguous()
    h = side / int(res)
    bvh = None
    if accel == 'bvh':                                                     # one tree for both queries
        from . import raytrace as _rt
        bvh = _rt.Bvh(v, f)
    sdf, _ = _mo.mesh_wsdf(pos, v, f, want_w=False, accel=accel, bvh=bvh)
    out = _mtets.marching_tets(pos, sdf, torch.ones_like(sdf), tets)
    wv, wf = out['verts_wt'].detach().contiguous(), out['faces_wt'].long().contiguous()
    if wf.shape[0] == 0:
        raise RuntimeError(f'watertight: nothing extracted at res = {res} (is the mesh consistently wound?)')
    if bvh is not None:                                                    # the cap test needs no sign: the nearest walk alone
        return wv, wf, bvh.nearest(wv).d2 > (h / 4) ** 2, h
    dist, _ = _mo.mesh_wsdf(wv, v, f, want_w=False)
    return wv, wf, dist.abs() > h / 4, h


def watertight(v, f, res=128, scale=1.1, relax_iters=32, accel='brute'):
    wv, wf, cap, _ = extract(v, f, res, scale, accel)
    return _mr.relax(wv, wf, cap, relax_iters), wf, cap
