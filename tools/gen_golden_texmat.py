"""Write tests/golden/tangents.npz: the reference's render/mesh.py compute_tangents (:452-495), run on the CPU in float64 and float32, on a small
mesh made here -- inputs and results, nothing else.  tests/texmat_cases.py reads only the .npz.

The mesh: a bumped 5 x 5 lattice (32 triangles) with
  * a uv chart of its own (a sheared planar map; the lattice's last column has duplicated uv vertices, so t_tex_idx != t_pos_idx),
  * split normals (the vertices of the middle row carry two normals, one per side: t_nrm_idx != t_pos_idx, every normal named by a triangle),
  * triangle 5 mirrored in the chart (two of its uv indices swapped onto uv vertices of their own: a negative denominator),
  * triangle 11 with its three uv indices on ONE uv vertex (numerator and denominator both zero: the -1e-6 clamp decides).
Both call forms are recorded: compute_tangents(mesh) and compute_tangents(mesh, v_tng=given).  Normals are supplied (the reference's auto_normals
hard-codes 'cuda')."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import refharness  # noqa: E402
from gen_golden import _savez_reproducible  # noqa: E402


def make_mesh():
    rng = np.random.default_rng(20240611)
    n = 5
    gx, gy = np.meshgrid(np.linspace(-1.0, 1.0, n), np.linspace(-1.0, 1.0, n), indexing='xy')
    z = 0.3 * np.sin(2.0 * gx) * np.cos(1.5 * gy) + 0.05 * rng.standard_normal(gx.shape)
    v_pos = np.stack([gx, gy, z], -1).reshape(-1, 3)
    vid = lambda i, j: j * n + i
    faces = []
    for j in range(n - 1):
        for i in range(n - 1):
            faces += [[vid(i, j), vid(i + 1, j), vid(i + 1, j + 1)], [vid(i, j), vid(i + 1, j + 1), vid(i, j + 1)]]
    t_pos = np.array(faces, np.int64)
    # uv chart: sheared planar map; the last column of the lattice gets a second set of uv vertices used by the triangles of the last cell column
    uv = np.stack([0.1 + 0.35 * (gx + 1) + 0.05 * (gy + 1), 0.15 + 0.3 * (gy + 1) + 0.04 * np.sin(3 * gx)], -1).reshape(-1, 2)
    v_tex = list(uv)
    t_tex = t_pos.copy()
    dup = {}
    for f, tri in enumerate(t_pos):
        if all(v % n >= n - 2 for v in tri):
            for k, v in enumerate(tri):
                if v % n == n - 1:
                    if v not in dup:
                        dup[v] = len(v_tex)
                        v_tex.append(uv[v] + np.array([0.013, -0.007]))
                    t_tex[f, k] = dup[v]
    # triangle 5: mirrored (corners 1 and 2 read each other's uv, through uv vertices of their own)
    a, b = t_tex[5, 1], t_tex[5, 2]
    t_tex[5, 1], t_tex[5, 2] = len(v_tex), len(v_tex) + 1
    v_tex += [np.array(v_tex[b]), np.array(v_tex[a])]
    # triangle 11: all three uvs coincide
    t_tex[11, :] = len(v_tex)
    v_tex.append(np.array([0.4321, 0.6789]))
    v_tex = np.array(v_tex)
    # normals: the smooth ones, and a second normal for the middle row used by the triangles above it
    nrm = np.stack([-0.6 * np.cos(2.0 * gx) * np.cos(1.5 * gy), 0.45 * np.sin(2.0 * gx) * np.sin(1.5 * gy), np.ones_like(gx)], -1).reshape(-1, 3)
    nrm += 0.05 * rng.standard_normal(nrm.shape)
    v_nrm = list(nrm / np.linalg.norm(nrm, axis=-1, keepdims=True))
    t_nrm = t_pos.copy()
    mid = n // 2
    second = {}
    for f, tri in enumerate(t_pos):
        if min(v // n for v in tri) >= mid:                     # a triangle above the middle row
            for k, v in enumerate(tri):
                if v // n == mid:
                    if v not in second:
                        second[v] = len(v_nrm)
                        m = v_nrm[v] + np.array([0.0, 0.35, 0.1])
                        v_nrm.append(m / np.linalg.norm(m))
                    t_nrm[f, k] = second[v]
    v_nrm = np.array(v_nrm)
    assert len(t_pos) < 100 and (t_nrm != t_pos).any() and (t_tex != t_pos).any() and set(t_nrm.reshape(-1)) == set(range(len(v_nrm)))
    given = rng.standard_normal(v_nrm.shape)
    return v_pos, t_pos, v_nrm, t_nrm, v_tex, t_tex, given


def main():
    v_pos, t_pos, v_nrm, t_nrm, v_tex, t_tex, given = make_mesh()
    out = {'v_pos': v_pos, 't_pos_idx': t_pos, 'v_nrm': v_nrm, 't_nrm_idx': t_nrm, 'v_tex': v_tex, 't_tex_idx': t_tex, 'v_tng_given': given}
    with refharness.ref_ctx():
        from render import mesh as rmesh
        assert rmesh.__file__.startswith(refharness.REF)
        for name, dt in (('f64', torch.float64), ('f32', torch.float32)):
            T = lambda a: torch.from_numpy(a).to(dt)
            I = lambda a: torch.from_numpy(a)
            m = rmesh.Mesh(T(v_pos), I(t_pos), T(v_nrm), I(t_nrm), T(v_tex), I(t_tex))
            r = rmesh.compute_tangents(m)
            assert torch.equal(r.t_tng_idx, I(t_nrm)) and r.v_tng.dtype == dt and bool(torch.isfinite(r.v_tng).all())
            out[f'tng.{name}'] = r.v_tng.numpy()
            out[f'tng_given.{name}'] = rmesh.compute_tangents(m, v_tng=T(given)).v_tng.numpy()
    e1, e2 = v_tex[t_tex[:, 1]] - v_tex[t_tex[:, 0]], v_tex[t_tex[:, 2]] - v_tex[t_tex[:, 0]]
    den = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    assert den[5] < 0 and den[11] == 0 and (np.delete(den, [5, 11]) > 0).all(), den
    print('tangents: %d faces, %d vertices, %d normals, %d uvs; f32 vs f64 %.2e' % (len(t_pos), len(v_pos), len(v_nrm), len(v_tex),
                                                                                  np.abs(out['tng.f32'] - out['tng.f64']).max()))
    _savez_reproducible(os.path.join(ROOT, 'tests', 'golden', 'tangents.npz'), out)


if __name__ == '__main__':
    main()
