"""Check functions of the 2-D material path -- render/mesh.py:compute_tangents, the per-pixel material lookup (csrc/texmat.hip, d3h/texmat.py), the
texture-map branch of render.render.render_mesh, d3h.export.load_textured_mesh -- shared by tests/test_texmat_emul.py (host emulation of the kernel
sources) and tests/test_gpu_texmat.py (MI355X).  Same shapes on both: synth.icosphere(1) scaled by 0.6, B = 2 frames of 37 x 53 pixels (tail threads,
a batch stride, more than one block), maps of at most 64 x 64.

Yardsticks are the float64 / float32 torch restatements below (texel coordinate, bilinear lookup, jitter tap, shading normal, tangents, the
barycentrics of a pixel as a function of the clip positions).  Parity rule for float tensors (tests/uvatlas_cases.py:assert_close):
max|got - f64| / max|f64| <= max(5 * ref32_err, 2^-20), ref32_err the distance of the float32 evaluation of the same yardstick.  Every figure is
printed before it is asserted (run with -s).

Composite + antialias are not restated: comparisons against a restatement are made on INTERIOR pixels (the pixel and its four neighbours covered) --
the mesh is convex and closed, so the only silhouette edges antialias blends across lie between a covered and an uncovered pixel -- and losses carry
zero weight elsewhere, so no gradient passes through a blended pixel."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from conftest import golden
from uvatlas_cases import FLOOR, _PositionAsColour, assert_close, assert_floor, rel

B, H, W = 2, 37, 53
TEX = 64


class _Flags:
    pass


def _t(a, dev, dtype=None):
    return torch.as_tensor(a, dtype=dtype).to(dev)


# ---- restatements (dtype-generic torch, differentiable) ----------------------------------------------------------------------------------
def y_normalize(x, eps=1e-20):
    return x / torch.sqrt(torch.clamp((x * x).sum(-1, keepdim=True), min=eps))


def y_tangents(v_pos, t_pos, v_nrm, t_nrm, v_tex, t_tex, v_tng=None):
    """compute_tangents of the upstream project, restated: [V,3] positions / normals of one frame"""
    if v_tng is None:
        p = [v_pos[t_pos[:, i]] for i in range(3)]
        t = [v_tex[t_tex[:, i]] for i in range(3)]
        u1, u2, p1, p2 = t[1] - t[0], t[2] - t[0], p[1] - p[0], p[2] - p[0]
        nom = p1 * u2[:, 1:2] - p2 * u1[:, 1:2]
        den = u1[:, 0:1] * u2[:, 1:2] - u1[:, 1:2] * u2[:, 0:1]
        tang = nom / torch.where(den > 0, den.clamp(min=1e-6), den.clamp(max=-1e-6))
        acc, cnt = torch.zeros_like(v_nrm), torch.zeros_like(v_nrm)
        for i in range(3):
            acc = acc.index_add(0, t_nrm[:, i], tang)
            cnt = cnt.index_add(0, t_nrm[:, i], torch.ones_like(tang))
        v_tng = acc / cnt
    v_tng = y_normalize(v_tng)
    return y_normalize(v_tng - (v_tng * v_nrm).sum(-1, keepdim=True) * v_nrm)


def y_interp(attr, rast, tri):
    """attr [V,A] or [B,V,A], rast [B,H,W,4] (already of attr's dtype), tri [F,3] -> [B,H,W,A]: u a0 + v a1 + (1 - u - v) a2, zeros where empty"""
    ids = rast[..., 3].long()
    f = (ids - 1).clamp(min=0)
    if attr.dim() == 3 and attr.shape[0] > 1:
        bi = torch.arange(rast.shape[0])[:, None, None].expand(ids.shape)
        a = attr[bi[..., None], tri[f]]
    else:
        a = (attr[0] if attr.dim() == 3 else attr)[tri[f]]
    u, v = rast[..., 0:1], rast[..., 1:2]
    out = u * a[..., 0, :] + v * a[..., 1, :] + (1 - u - v) * a[..., 2, :]
    return torch.where((ids > 0)[..., None], out, torch.zeros_like(out))


def y_bilinear(tex, uv, boundary='wrap'):
    """level-0 bilinear lookup: tex [1,h,w,C], uv [B,H,W,2]; texel centres at (i + 0.5) / N, taps wrapped (positive modulo) or clamped"""
    h, w = tex.shape[1:3]
    x, y = uv[..., 0] * w - 0.5, uv[..., 1] * h - 0.5
    xf, yf = torch.floor(x), torch.floor(y)
    fx, fy = (x - xf)[..., None], (y - yf)[..., None]
    bound = (lambda i, n: torch.remainder(i, n)) if boundary == 'wrap' else (lambda i, n: i.clamp(0, n - 1))
    x0, x1, y0, y1 = bound(xf.long(), w), bound(xf.long() + 1, w), bound(yf.long(), h), bound(yf.long() + 1, h)
    t = lambda yy, xx: tex[0][yy, xx]
    return (t(y0, x0) * (1 - fx) + t(y0, x1) * fx) * (1 - fy) + (t(y1, x0) * (1 - fx) + t(y1, x1) * fx) * fy


def y_lookup(rast, v_tex, tri, maps, boundary, dtype):
    """the fused lookup: one image per map, zeros at empty pixels"""
    r = rast.to(dtype)
    uv = y_interp(v_tex.to(dtype), r, tri)
    hit = (r[..., 3:4] > 0).to(dtype)
    return [y_bilinear(m.to(dtype) if m.dtype != dtype else m, uv, boundary) * hit for m in maps]


def y_tap(img, offset):
    """bilinear / clamp lookup of an image [B,H,W,C] at the jittered pixel grid: pixel centres + offset (in [-1, 1] units of render.util.pixel_grid)"""
    Bn, Hn, Wn = img.shape[:3]
    gy, gx = torch.meshgrid((torch.arange(Hn, dtype=img.dtype) + 0.5) / Hn, (torch.arange(Wn, dtype=img.dtype) + 0.5) / Wn, indexing='ij')
    uv = torch.stack((gx, gy), -1)[None] + offset.to(img.dtype)
    x, y = uv[..., 0] * Wn - 0.5, uv[..., 1] * Hn - 0.5
    xf, yf = torch.floor(x), torch.floor(y)
    fx, fy = (x - xf)[..., None], (y - yf)[..., None]
    x0, x1, y0, y1 = xf.long().clamp(0, Wn - 1), (xf.long() + 1).clamp(0, Wn - 1), yf.long().clamp(0, Hn - 1), (yf.long() + 1).clamp(0, Hn - 1)
    bi = torch.arange(Bn)[:, None, None].expand(x0.shape)
    t = lambda yy, xx: img[bi, yy, xx]
    return (t(y0, x0) * (1 - fx) + t(y0, x1) * fx) * (1 - fy) + (t(y1, x0) * (1 - fx) + t(y1, x1) * fx) * fy


def y_shading_normal(pos, view_pos, pert, snrm, stng, gnrm):
    """prepare_shading_normal (two-sided, OpenGL bitangent) of the upstream project's python twin, restated"""
    dot = lambda a, b: (a * b).sum(-1, keepdim=True)
    sn, st, vv = y_normalize(snrm), y_normalize(stng), y_normalize(view_pos - pos)
    if pert is None:
        pert = torch.tensor([0.0, 0.0, 1.0], dtype=pos.dtype).expand(pos.shape)
    bt = y_normalize(torch.cross(st, sn, dim=-1))
    sh = y_normalize(st * pert[..., 0:1] - bt * pert[..., 1:2] + sn * pert[..., 2:3].clamp(min=0.0))
    front = dot(gnrm, vv) > 0
    sh, g = torch.where(front, sh, -sh), torch.where(front, gnrm, -gnrm)
    t = (dot(vv, sh) / 0.1).clamp(0, 1)
    return g + t * (sh - g)


def y_rast_uv(clip, tri, rast):
    """the barycentrics (u, v) of every covered pixel centre as a differentiable function of the clip positions clip [B,V,4] (the triangle of each
    pixel taken from `rast`): b_i proportional to the cross products of q_j = (X_j - x W_j, Y_j - y W_j), perspective-correct"""
    Bn, Hn, Wn = rast.shape[:3]
    ids = rast[..., 3].long()
    f = (ids - 1).clamp(min=0)
    bi = torch.arange(Bn)[:, None, None].expand(ids.shape)
    P = clip[bi[..., None], tri[f]]                                    # [B,H,W,3,4]
    x = ((torch.arange(Wn, dtype=clip.dtype) + 0.5) / Wn * 2 - 1)[None, None, :, None]
    y = ((torch.arange(Hn, dtype=clip.dtype) + 0.5) / Hn * 2 - 1)[None, :, None, None]
    qx, qy = P[..., 0] - x * P[..., 3], P[..., 1] - y * P[..., 3]
    cr = lambda i, j: qx[..., i] * qy[..., j] - qx[..., j] * qy[..., i]
    b0, b1, b2 = cr(1, 2), cr(2, 0), cr(0, 1)
    s = b0 + b1 + b2
    s = torch.where(ids > 0, s, torch.ones_like(s))
    return torch.stack((b0 / s, b1 / s), -1)


# ---- the scene ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _scene_np():
    from d3h import synth
    from render import util
    v, t = synth.icosphere(1)
    v = (np.asarray(v, np.float32) * np.float32(0.6)).astype(np.float32)
    proj = util.perspective(0.6, W / H, 0.1, 10.0)
    mv0, mv1 = util.translate(0.0, 0.0, -2.5) @ util.rotate_y(0.4), util.translate(0.12, -0.05, -2.2) @ util.rotate_y(-0.9)
    mvp = torch.stack([proj @ mv0, proj @ mv1]).float()
    cam = torch.stack([torch.linalg.inv(mv0)[:3, 3], torch.linalg.inv(mv1)[:3, 3]]).float()
    g = torch.Generator().manual_seed(5)
    draws = {'noise': torch.randn(B, H, W, 3, generator=g), 'offset': torch.randn(B, H, W, 2, generator=g) * 0.005,
             'pos_noise': torch.randn(B, H, W, 3, generator=g) * 0.01}
    return v, np.asarray(t, np.int64), mvp, cam, draws


def scene(dev, tilt=None, res=TEX):
    """-> (base mesh with the stand-in MLP material, exported mesh with tangents, mvp, campos, draws).  `tilt`: the constant the normal map is set to"""
    from d3h import export
    from render import mesh as rmesh
    v, t, mvp, cam, draws = _scene_np()
    mat = {'bsdf': 'pbr', 'kd_ks': _PositionAsColour()}
    base = rmesh.auto_normals(rmesh.Mesh(_t(v, dev), _t(t, dev), material=mat))
    ex = export.textured_mesh(base, mat, res, [-1.0] * 3, [1.0] * 3, [-1.0] * 3, [1.0] * 3, [-1.0, -1.0, 0.0], [1.0, 1.0, 1.0])
    ex = rmesh.compute_tangents(ex)
    if tilt is not None:
        with torch.no_grad():
            ex.material['normal'].data.copy_(_t(tilt, dev, torch.float32).expand_as(ex.material['normal'].data))
    return base, ex, mvp.to(dev), cam.to(dev), draws


def render(mesh, mesh_original, mvp, cam, draws, fused=None, **kw):
    """render_mesh under fixed draws; fused None: the default route, True / False: D3H_TEXMAT_FUSED forced"""
    import nvdiffrast.torch as dr
    from render import render as rr
    old = os.environ.get('D3H_TEXMAT_FUSED')
    if fused is not None:
        os.environ['D3H_TEXMAT_FUSED'] = '1' if fused else '0'
    try:
        return rr.render_mesh(_Flags(), 0, dr.RasterizeGLContext(), mesh, mesh_original, mvp, cam, None, [H, W], _rng_draws=draws, **kw)
    finally:
        if fused is not None:
            if old is None:
                del os.environ['D3H_TEXMAT_FUSED']
            else:
                os.environ['D3H_TEXMAT_FUSED'] = old


def interior(rast):
    """[B,H,W] bool: the pixel and its four neighbours are covered"""
    c = (rast[..., 3] > 0).cpu()
    m = c.clone()
    m[:, 1:] &= c[:, :-1]
    m[:, :-1] &= c[:, 1:]
    m[:, :, 1:] &= c[:, :, :-1]
    m[:, :, :-1] &= c[:, :, 1:]
    m[:, 0] = m[:, -1] = False
    m[:, :, 0] = m[:, :, -1] = False
    return m


def routes_taken(fn):
    """run fn() and report which lookup route render_mesh took: {'fused': n, 'composed': n}"""
    from d3h import texmat
    from render import render as rr
    n = {'fused': 0, 'composed': 0}
    f0, i0 = texmat.lookup, rr.interpolate

    def f1(*a, **k):
        n['fused'] += 1
        return f0(*a, **k)

    def i1(attr, *a, **k):
        if attr.shape[-1] == 2:
            n['composed'] += 1
        return i0(attr, *a, **k)
    texmat.lookup, rr.interpolate = f1, i1
    try:
        out = fn()
    finally:
        texmat.lookup, rr.interpolate = f0, i0
    return out, n


# ---- 1. tangents -------------------------------------------------------------------------------------------------------------------------
def _golden_mesh(dev, G, dtype=torch.float32):
    from render import mesh as rmesh
    T = lambda k: torch.from_numpy(G[k]).to(dtype).to(dev)
    I = lambda k: torch.from_numpy(G[k]).to(dev)
    return rmesh.Mesh(T('v_pos'), I('t_pos_idx'), T('v_nrm'), I('t_nrm_idx'), T('v_tex'), I('t_tex_idx'))


def check_tangents_golden(dev):
    from render import mesh as rmesh
    G = golden('tangents.npz')
    m = _golden_mesh(dev, G)
    assert len(G['t_pos_idx']) < 100 and (G['t_nrm_idx'] != G['t_pos_idx']).any() and (G['t_tex_idx'] != G['t_pos_idx']).any()
    r = rmesh.compute_tangents(m)
    assert r.t_tng_idx is m.t_nrm_idx and r.v_tng.shape == m.v_nrm.shape and r.v_pos is m.v_pos and r.v_tex is m.v_tex
    assert_close('compute_tangents vs the upstream float64 run', r.v_tng, G['tng.f64'], G['tng.f32'])
    given = torch.from_numpy(G['v_tng_given']).float().to(dev)
    r2 = rmesh.compute_tangents(m, v_tng=given)
    assert r2.t_tng_idx is m.t_nrm_idx
    assert_close('compute_tangents(v_tng=given) vs the upstream float64 run', r2.v_tng, G['tng_given.f64'], G['tng_given.f32'])
    # the restatement agrees with upstream too (it is the yardstick of the gradient check)
    a = [torch.from_numpy(G[k]) for k in ('v_pos', 't_pos_idx', 'v_nrm', 't_nrm_idx', 'v_tex', 't_tex_idx')]
    assert rel(y_tangents(*a), G['tng.f64']) < 1e-12 and rel(y_tangents(*a, v_tng=torch.from_numpy(G['v_tng_given'])), G['tng_given.f64']) < 1e-12
    assert float((r.v_tng * m.v_nrm).sum(-1).abs().max()) < 1e-5 and float((r.v_tng.norm(dim=-1) - 1).abs().max()) < 1e-5


def check_tangents_batched(dev):
    from render import mesh as rmesh
    G = golden('tangents.npz')
    m = _golden_mesh(dev, G)
    g = torch.Generator().manual_seed(3)
    pos2 = m.v_pos + 0.1 * torch.randn(m.v_pos.shape, generator=g).to(dev)
    nrm2 = y_normalize(m.v_nrm + 0.2 * torch.randn(m.v_nrm.shape, generator=g).to(dev))
    frames = [(m.v_pos, m.v_nrm), (pos2, nrm2)]
    both = rmesh.compute_tangents(rmesh.Mesh(torch.stack([p for p, _ in frames]), v_nrm=torch.stack([n for _, n in frames]), base=m))
    assert both.v_tng.shape == (2,) + tuple(m.v_nrm.shape)
    given = torch.from_numpy(G['v_tng_given']).float().to(dev)
    both_given = rmesh.compute_tangents(rmesh.Mesh(torch.stack([p for p, _ in frames]), v_nrm=torch.stack([n for _, n in frames]), base=m),
                                        v_tng=torch.stack([given, given]))
    for b, (p, n) in enumerate(frames):
        one = rmesh.Mesh(p, v_nrm=n, base=m)
        assert_floor(f'batched tangents, frame {b}, vs the per-frame call', both.v_tng[b], rmesh.compute_tangents(one).v_tng)
        assert_floor(f'batched tangents with v_tng given, frame {b}', both_given.v_tng[b], rmesh.compute_tangents(one, v_tng=given).v_tng)


def check_tangents_gradient(dev):
    from render import mesh as rmesh
    G = golden('tangents.npz')
    wgt = torch.randn(G['v_nrm'].shape, generator=torch.Generator().manual_seed(9), dtype=torch.float64)
    m = _golden_mesh(dev, G)
    m.v_pos = m.v_pos.clone().requires_grad_(True)
    m.v_nrm = m.v_nrm.clone().requires_grad_(True)
    (rmesh.compute_tangents(m).v_tng * wgt.float().to(dev)).sum().backward()
    ref = {}
    for dt in (torch.float64, torch.float32):
        a = [torch.from_numpy(G[k]) for k in ('v_pos', 't_pos_idx', 'v_nrm', 't_nrm_idx', 'v_tex', 't_tex_idx')]
        a = [x.to(dt) if x.is_floating_point() else x for x in a]
        a[0].requires_grad_(True)
        a[2].requires_grad_(True)
        (y_tangents(*a) * wgt.to(dt)).sum().backward()
        ref[dt] = (a[0].grad, a[2].grad)
    assert float(ref[torch.float64][0].abs().max()) > 0
    assert_close('d tangents / d v_pos vs float64 autograd', m.v_pos.grad, ref[torch.float64][0], ref[torch.float32][0])
    assert_close('d tangents / d v_nrm vs float64 autograd', m.v_nrm.grad, ref[torch.float64][1], ref[torch.float32][1])


def check_mesh_helpers(dev, tmp_path):
    from render import mesh as rmesh, obj
    G = golden('tangents.npz')
    m = _golden_mesh(dev, G)
    lo, hi = rmesh.aabb(m)
    assert torch.equal(lo, m.v_pos.min(0).values) and torch.equal(hi, m.v_pos.max(0).values)
    u = rmesh.unit_size(m)
    ulo, uhi = rmesh.aabb(u)
    assert abs(float((uhi - ulo).max()) - 2.0) < 1e-5 and float((uhi + ulo).abs().max()) < 1e-5 and u.t_pos_idx is m.t_pos_idx
    c = rmesh.center_by_reference(m, (lo.cpu(), hi.cpu()), 3.0)
    clo, chi = rmesh.aabb(c)
    assert c.v_pos.device == m.v_pos.device and abs(float((chi - clo).max()) - 3.0) < 1e-5 and float((chi + clo).abs().max()) < 1e-5
    obj.write_obj(str(tmp_path), m)
    back = rmesh.load_mesh(os.path.join(str(tmp_path), 'mesh.obj'))
    assert back.v_pos.shape == m.v_pos.shape and torch.equal(back.t_pos_idx.cpu(), m.t_pos_idx.cpu()) and torch.equal(back.t_nrm_idx.cpu(), m.t_nrm_idx.cpu())


# ---- 2. the lookup kernel ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _lookup_inputs():
    """a synthetic raster over F = 23 triangles: random barycentrics, a third of the pixels empty, uvs reaching outside [0, 1]; the first pixels sit exactly on
    a vertex (u = 1: the texel coordinate IS that vertex's uv) whose uv is a texel centre, a texel edge or a corner of the 16-grid, in and out of range"""
    g = torch.Generator().manual_seed(17)
    F, Vt = 23, 40
    tri = torch.stack([torch.randperm(Vt, generator=g)[:3] for _ in range(F)]).int()
    v_tex = torch.rand(Vt, 2, generator=g) * 2.6 - 0.8
    special = torch.tensor([[3.5 / 16, 8.5 / 16], [4.0 / 16, 8.0 / 16], [0.0, 0.0], [1.0, 1.0], [-0.25, 1.5], [0.5 / 16, 15.5 / 16], [1.0 + 0.5 / 16, -0.5 / 16],
                            [0.5, 0.5 / 32]])
    bar = torch.from_numpy(np.random.default_rng(17).dirichlet((1.0, 1.0, 1.0), (B, H, W))).float()
    ids = torch.randint(0, F + 1, (B, H, W), generator=g)
    ids[torch.rand(B, H, W, generator=g) < 0.3] = 0
    rast = torch.stack([bar[..., 0], bar[..., 1], torch.rand(B, H, W, generator=g), ids.float()], -1)
    for k in range(len(special)):                      # pixel (0, 0, k) and (1, H-1, W-1-k): u = 1 on a vertex that carries special[k]
        v_tex[tri[k, 0].long()] = special[k]
        for b, y, x in ((0, 0, k), (1, H - 1, W - 1 - k)):
            rast[b, y, x] = torch.tensor([1.0, 0.0, 0.5, k + 1.0])
    maps = [torch.rand(1, 16, 16, 3, generator=g), torch.rand(1, 8, 32, 3, generator=g), torch.rand(1, 1, 1, 3, generator=g)]
    wgts = [torch.rand(B, H, W, 3, generator=g) + 0.5 for _ in maps]
    return rast, v_tex, tri, maps, wgts


def check_lookup(dev, boundary):
    import nvdiffrast.torch as dr
    from d3h import texmat
    rast, v_tex, tri, maps, wgts = _lookup_inputs()
    assert int((rast[..., 3] == 0).sum()) > 0.2 * B * H * W and float(v_tex.min()) < -0.5 and float(v_tex.max()) > 1.5
    d = lambda x: x.to(dev)
    leaf = [d(m).clone().requires_grad_(True) for m in maps]
    got = texmat.lookup(d(rast), d(v_tex), d(tri), leaf, boundary=boundary)
    assert [tuple(o.shape) for o in got] == [(B, H, W, 3)] * 3
    sum((o * d(w)).sum() for o, w in zip(got, wgts)).backward()
    # the composed route: interpolate, then one texture lookup per map, masked (an empty pixel has texel coordinate (0, 0) there)
    comp_leaf = [d(m).clone().requires_grad_(True) for m in maps]
    texc, _ = dr.interpolate(d(v_tex)[None].contiguous(), d(rast), d(tri))
    hit = (d(rast)[..., 3:4] > 0).float()
    comp = [dr.texture(m, texc, filter_mode='linear', boundary_mode=boundary) * hit for m in comp_leaf]
    sum((o * d(w)).sum() for o, w in zip(comp, wgts)).backward()
    ref = {}
    for dt in (torch.float64, torch.float32):
        ms = [m.to(dt).clone().requires_grad_(True) for m in maps]
        outs = y_lookup(rast, v_tex, tri.long(), ms, boundary, dt)
        sum((o * w.to(dt)).sum() for o, w in zip(outs, wgts)).backward()
        ref[dt] = ([o.detach() for o in outs], [m.grad for m in ms])
    empty = (rast[..., 3] == 0)
    for i, name in enumerate(('kd 16x16', 'ks 8x32', 'normal 1x1')):
        assert not got[i].detach().cpu()[empty].any(), 'an empty pixel is not zero'
        assert_close(f'fused lookup [{boundary}] {name} vs float64', got[i], ref[torch.float64][0][i], ref[torch.float32][0][i])
        assert_close(f'composed lookup [{boundary}] {name} vs float64', comp[i], ref[torch.float64][0][i], ref[torch.float32][0][i])
        assert_floor(f'fused vs composed [{boundary}] {name}', got[i], comp[i].detach())
        assert_close(f'fused map gradient [{boundary}] {name} vs float64', leaf[i].grad, ref[torch.float64][1][i], ref[torch.float32][1][i])
        assert_close(f'composed map gradient [{boundary}] {name} vs float64', comp_leaf[i].grad, ref[torch.float64][1][i], ref[torch.float32][1][i])
    # a single map, and two maps of one resolution (shared taps)
    one = texmat.lookup(d(rast), d(v_tex), d(tri), [d(maps[1])], boundary=boundary)
    assert torch.equal(one[0], got[1].detach())
    twin = texmat.lookup(d(rast), d(v_tex), d(tri), [d(maps[0]), d(maps[1]), d(maps[0]) * 2], boundary=boundary)
    assert torch.equal(twin[0], got[0].detach()) and torch.equal(twin[1], got[1].detach())
    assert_floor('third map on the taps of the first', twin[2], got[0].detach() * 2)


def check_lookup_grad_buffers(dev):
    """a map that does not require grad gets no gradient buffer (and no gradient)"""
    from d3h import texmat, _lib as L
    rast, v_tex, tri, maps, wgts = _lookup_inputs()
    d = lambda x: x.to(dev)
    kd, ks, nrm = d(maps[0]).clone().requires_grad_(True), d(maps[1]).clone(), d(maps[2]).clone().requires_grad_(True)
    made = []
    z0 = L.zeros_like
    L.zeros_like = lambda t, dtype=None: (made.append(tuple(t.shape)), z0(t, dtype))[1]
    try:
        outs = texmat.lookup(d(rast), d(v_tex), d(tri), [kd, ks, nrm])
        (outs[0].sum() + outs[1].sum() + outs[2].sum()).backward()
    finally:
        L.zeros_like = z0
    assert sorted(made) == sorted([tuple(kd.shape), tuple(nrm.shape)]), made
    assert kd.grad is not None and nrm.grad is not None and ks.grad is None
    with pytest.raises(ValueError):
        texmat.lookup(d(rast).clone().requires_grad_(True), d(v_tex), d(tri), [kd])
    with pytest.raises(ValueError):
        texmat.lookup(d(rast), d(v_tex), d(tri), [kd, ks, nrm, kd])
    with pytest.raises(ValueError):
        texmat.lookup(d(rast), d(v_tex), d(tri), [torch.zeros(1, 4, 4, 5, device=dev)])


def check_lookup_empty(dev):
    from d3h import texmat
    rast, v_tex, tri, maps, _ = _lookup_inputs()
    d = lambda x: x.to(dev)
    leaf = d(maps[0]).clone().requires_grad_(True)
    out = texmat.lookup(d(rast), d(v_tex), torch.zeros(0, 3, dtype=torch.int32, device=dev), [leaf, d(maps[2])])     # F = 0: every id is past the face list
    assert [tuple(o.shape) for o in out] == [(B, H, W, 3)] * 2 and not out[0].any() and not out[1].any()
    out[0].sum().backward()
    assert leaf.grad is not None and not leaf.grad.any()
    none = texmat.lookup(torch.zeros(0, H, W, 4, device=dev), d(v_tex), d(tri), [d(maps[0])])                          # B H W = 0
    assert tuple(none[0].shape) == (0, H, W, 3)


def check_lookup_entry_points_validate(dev):
    """argument errors come back as codes, not as launches"""
    from d3h import _lib as L
    lib = L.lib()
    rast = torch.zeros(1, 2, 2, 4, device=dev)
    rast[..., 3] = 1
    v_tex, tri = torch.zeros(3, 2, device=dev), torch.tensor([[0, 1, 2]], dtype=torch.int32, device=dev)
    tex, out, g = torch.zeros(1, 4, 4, 4, device=dev), torch.zeros(1, 2, 2, 4, device=dev), torch.zeros(1, 2, 2, 4, device=dev)
    p = lambda t: L._PTR(t.data_ptr())
    arr = lambda *ts: (ctypes.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])
    hwc = lambda *v: (ctypes.c_int * len(v))(*v)

    def fwd(rast_p=p(rast), vt=p(v_tex), tr=p(tri), F=1, npix=4, n=1, texs=arr(tex), sizes=hwc(4, 4, 4), bnd=0, outs=arr(out)):
        return lib.d3h_texmat_fwd(rast_p, vt, L.i64(3), tr, L.i64(F), L.i64(npix), L.i32(n), texs, sizes, L.i32(bnd), outs, L.stream())

    def bwd(n=1, texs=arr(tex), sizes=hwc(4, 4, 4), gs=arr(g), ds=arr(tex), F=1, npix=4):
        return lib.d3h_texmat_bwd(p(rast), p(v_tex), L.i64(3), p(tri), L.i64(F), L.i64(npix), L.i32(n), texs, sizes, L.i32(0), gs, ds, L.stream())
    assert fwd() == 0 and bwd() == 0
    assert fwd(rast_p=None) == -1 and fwd(vt=None) == -1 and fwd(tr=None) == -1 and fwd(texs=None) == -1 and fwd(sizes=None) == -1 and fwd(outs=None) == -1
    assert fwd(texs=arr(None)) == -1 and fwd(outs=arr(None)) == -1
    assert fwd(sizes=hwc(4, 4, 5)) == -1                                                     # C > 4
    assert fwd(sizes=hwc(0, 4, 4)) == -1 and fwd(sizes=hwc(4, -1, 4)) == -1 and fwd(sizes=hwc(4, 4, 0)) == -1
    assert fwd(n=4, texs=arr(tex, tex, tex, tex), sizes=hwc(*[4] * 12), outs=arr(out, out, out, out)) == -1      # more than 3 maps
    assert fwd(n=0) == -1 and fwd(bnd=2) == -1 and fwd(F=-1) == -1 and fwd(npix=-1) == -1
    assert fwd(rast_p=L._PTR(rast.data_ptr() + 4)) == -1                                     # the raster is read 16 bytes at a time
    assert fwd(F=0, tr=None, vt=None) == 0 and fwd(npix=0, rast_p=None, outs=arr(None)) == 0  # valid, nothing launched
    assert bwd(gs=None) == -1 and bwd(ds=None) == -1 and bwd(gs=arr(None)) == -1 and bwd(sizes=hwc(4, 4, 5)) == -1 and bwd(n=4) == -1
    assert bwd(gs=arr(None), ds=arr(None)) == 0 and bwd(F=0) == 0 and bwd(npix=0) == 0
    if dev != 'cpu':
        torch.cuda.synchronize()
    L._keepalive.clear()


# ---- 3. the export renders as what was baked ---------------------------------------------------------------------------------------------
def check_export_renders_as_baked(dev):
    base, ex, mvp, cam, draws = scene(dev)
    assert ex.material['filter_mode'] == 'linear'
    with torch.no_grad():
        mlp = render(base, base, mvp, cam, draws, buffers=('kd', '_rast'))
        rast = mlp['_rast'].cpu()
        ins = interior(rast)
        assert int(ins.sum()) > 200 and int((rast[..., 3] == 0).sum()) > 200
        v, t, _, _, _ = _scene_np()
        tri = torch.from_numpy(t)
        tex_idx = ex.t_tex_idx.cpu()
        y64 = y_interp(torch.from_numpy(v).double(), rast.double(), tri)                       # the colour IS the surface position
        y32 = y_bilinear(ex.material['kd'].data.detach().cpu(), y_interp(ex.v_tex.cpu(), rast, tex_idx), 'wrap')     # float32 interpolate-then-bilinear
        exact = y_bilinear(ex.material['kd'].data.detach().cpu().double(), y_interp(ex.v_tex.cpu().double(), rast.double(), tex_idx), 'wrap')
        print(f'float64 interpolate-then-bilinear of the bake vs the position: {float((exact - y64)[ins].abs().max()):.3e}')
        assert float((exact - y64)[ins].abs().max()) <= 3.9e-7
        assert_close('MLP render kd, interior, vs the float64 position', mlp['kd'][..., :3].cpu()[ins], y64[ins], y32[ins])
        tol = max(5.0 * rel(y32[ins], y64[ins]), FLOOR)
        for fused in (True, False):
            (out, n) = routes_taken(lambda: render(ex, None, mvp, cam, draws, fused=fused, buffers=('kd',)))
            assert n == ({'fused': 1, 'composed': 0} if fused else {'fused': 0, 'composed': 1}), n
            what = 'fused' if fused else 'composed'
            assert_close(f'exported mesh kd [{what}], interior, vs the float64 position', out['kd'][..., :3].cpu()[ins], y64[ins], y32[ins])
            # whole buffers, antialiased pixels included: each render may sit `tol` from the exact colour, so the two are within 2 tol of each other
            r = rel(out['kd'], mlp['kd'])
            print(f'exported mesh kd [{what}] vs the MLP render, whole buffer: {r:.3e} (bound {2 * tol:.3e})')
            assert r <= 2 * tol
            assert torch.equal(out['kd'][..., 3], mlp['kd'][..., 3])
        # without the key the default (mip-mapped) lookup mixes triangles: the key is honoured
        del ex.material['filter_mode']
        (mip, n) = routes_taken(lambda: render(ex, None, mvp, cam, draws, buffers=('kd',)))
        assert n == {'fused': 0, 'composed': 1}
        worst = float((mip['kd'] - mlp['kd']).abs().max())
        print(f'the same render without filter_mode: off by up to {worst:.3f}')
        assert worst > 0.1
        ex.material['filter_mode'] = 'nearest'
        near = render(ex, None, mvp, cam, draws, buffers=('kd',))
        assert float((near['kd'] - mlp['kd']).abs().max()) < 0.6 * 2.5 / (TEX // 5)              # within a texel or so of the bake (cells of 12 texels span <= 0.6 x 2.5)


# ---- 4. branch behaviour -----------------------------------------------------------------------------------------------------------------
TILT = (0.3, -0.2, 0.8)


def _y_buffers(ex_np, rast, clip, maps, tilt_map, draws, cam, dtype, use_tangent=True, v_pos=None):
    """the restated layer (before composite / antialias): kd, ks, perturbed normal, shading normal and the three smoothness buffers.  v_pos / clip
    given as differentiable tensors make the barycentrics a function of them."""
    c = lambda a: torch.as_tensor(a).to(dtype)
    tri, tex_idx = ex_np['tri'], ex_np['t_tex_idx']
    r = rast.to(dtype)
    if clip is not None:
        r = torch.cat((y_rast_uv(clip, tri, rast), r[..., 2:]), -1)
    pos_v = c(ex_np['v_pos']) if v_pos is None else v_pos
    mask = (r[..., 3:4] > 0).to(dtype)
    uv = y_interp(c(ex_np['v_tex']), r, tex_idx)
    kd, ks, pert = (y_bilinear(m, uv, 'wrap') * mask for m in (maps[0], maps[1], tilt_map))
    gb_pos, gb_nrm = y_interp(pos_v, r, tri), y_interp(c(ex_np['v_nrm']), r, tri)
    fn = torch.cross(pos_v[tri[:, 1]] - pos_v[tri[:, 0]], pos_v[tri[:, 2]] - pos_v[tri[:, 0]], dim=-1)
    fn = y_normalize(fn)
    ids = rast[..., 3].long()
    gnrm = torch.where((ids > 0)[..., None], fn[(ids - 1).clamp(min=0)], torch.zeros_like(gb_pos))
    if use_tangent:
        tng = y_interp(c(ex_np['v_tng']), r, tri)
    else:
        noise = draws['noise'].to(dtype)
        tng = torch.cross(noise / noise.norm(dim=-1, keepdim=True), gb_nrm, dim=-1)
    view = c(cam)[:, None, None, :]
    normal = y_shading_normal(gb_pos, view, pert if use_tangent else None, gb_nrm, tng, gnrm)
    off = draws['offset']
    gw = mask * y_tap(mask, off)
    out = {'kd': kd, 'ks': ks, 'perturbed_nrm': pert, 'normal': normal, 'shaded': kd,
           'kd_grad': (y_tap(kd, off) - kd).abs() * gw, 'ks_grad': (y_tap(ks, off) - ks).abs() * gw * torch.tensor([0.0, 1.0, 1.0], dtype=dtype),
           'normal_grad': (y_tap(gb_nrm, off) - gb_nrm).abs() * gw}
    both = y_normalize(y_normalize(y_tap(pert, off)) + y_normalize(pert))
    out['perturbed_nrm_grad'] = (1.0 - both[..., 2:3]).repeat(1, 1, 1, 3) * gw
    return out


def _ex_np(ex):
    return {'v_pos': ex.v_pos.detach().cpu(), 'v_nrm': ex.v_nrm.detach().cpu(), 'v_tng': ex.v_tng.detach().cpu(), 'v_tex': ex.v_tex.cpu(),
            'tri': ex.t_pos_idx.cpu(), 't_tex_idx': ex.t_tex_idx.cpu()}


def _public(out):
    return sorted(k for k in out if not k.startswith('_') and k != 'visible_triangles')


def check_branch_buffers(dev):
    """which buffers exist when; the unperturbed and the tilted normal; the smoothness buffers against their restatements"""
    from render import render as rr
    base, ex, mvp, cam, draws = scene(dev)
    every = sorted(rr.ALL_BUFFERS + rr.PERTURBED_BUFFERS)
    with torch.no_grad():
        flat = render(ex, None, mvp, cam, draws, _keep_rast=True)
        assert _public(flat) == every
        rast = flat['_rast'].cpu()
        ins = interior(rast)
        # every way of switching the perturbation off: the two buffers are gone, the tangent is the random one
        plain = render(ex, None, mvp, cam, draws, use_uv=False)
        assert _public(plain) == sorted(rr.ALL_BUFFERS)
        assert _public(render(ex, None, mvp, cam, draws, finetune_normal=False)) == sorted(rr.ALL_BUFFERS)
        ex.material['no_perturbed_nrm'] = True
        assert _public(render(ex, None, mvp, cam, draws)) == sorted(rr.ALL_BUFFERS)
        ex.material['no_perturbed_nrm'] = False
        assert _public(render(ex, None, mvp, cam, draws)) == every
        del ex.material['no_perturbed_nrm']
        from render import mesh as rmesh
        no_tng = rmesh.Mesh(base=ex)
        no_tng.v_tng = no_tng.t_tng_idx = None
        assert _public(render(no_tng, None, mvp, cam, draws)) == sorted(rr.ALL_BUFFERS)
        nrm_map = ex.material.pop('normal')
        assert _public(render(ex, None, mvp, cam, draws)) == sorted(rr.ALL_BUFFERS)
        ex.material['normal'] = nrm_map
        assert _public(render(ex, None, mvp, cam, draws, buffers=('kd', 'perturbed_nrm'))) == ['kd', 'perturbed_nrm']
        assert _public(render(ex, None, mvp, cam, draws, buffers=('kd', 'perturbed_nrm'), use_uv=False)) == ['kd']
        # a constant (0, 0, 1) map: the shading normal of the unperturbed path (restated with the interpolated tangent, which drops out)
        E = _ex_np(ex)
        maps = [ex.material[k].data.detach().cpu() for k in ('kd', 'ks')]
        up = ex.material['normal'].data.detach().cpu()
        y = {dt: _y_buffers(E, rast, None, [m.to(dt) for m in maps], up.to(dt), draws, cam.cpu(), dt) for dt in (torch.float64, torch.float32)}
        y_plain = {dt: _y_buffers(E, rast, None, [m.to(dt) for m in maps], up.to(dt), draws, cam.cpu(), dt, use_tangent=False) for dt in (torch.float64, torch.float32)}
        I = lambda t: t[..., :3].cpu()[ins]
        assert_close('normal under a (0, 0, 1) map vs the unperturbed restatement', I(flat['normal']), y_plain[torch.float64]['normal'][ins], y_plain[torch.float32]['normal'][ins])
        assert_close('normal of the unperturbed render (use_uv=False)', I(plain['normal']), y_plain[torch.float64]['normal'][ins], y_plain[torch.float32]['normal'][ins])
        assert_close('perturbed_nrm under a (0, 0, 1) map', I(flat['perturbed_nrm']), y[torch.float64]['perturbed_nrm'][ins], y[torch.float32]['perturbed_nrm'][ins])
        assert float(I(flat['perturbed_nrm_grad']).abs().max()) <= 1e-6
    # a tilted constant map: the restatement of prepare_shading_normal with the interpolated tangent
    base, ex, mvp, cam, draws = scene(dev, tilt=TILT)
    with torch.no_grad():
        E = _ex_np(ex)
        tilt = ex.material['normal'].data.detach().cpu()
        y = {dt: _y_buffers(E, rast, None, [m.to(dt) for m in maps], tilt.to(dt), draws, cam.cpu(), dt) for dt in (torch.float64, torch.float32)}
        for fused in (True, False):
            out = render(ex, None, mvp, cam, draws, fused=fused)
            what = 'fused' if fused else 'composed'
            for k in ('normal', 'kd', 'ks', 'perturbed_nrm', 'kd_grad', 'ks_grad', 'normal_grad'):
                assert_close(f'{k} [{what}], tilted normal map, interior', I(out[k]), y[torch.float64][k][ins], y[torch.float32][k][ins])
            assert float((I(out['normal']) - I(flat['normal'])).abs().max()) > 0.05
            assert not I(out['ks_grad'])[..., 0].any() and float(I(out['kd_grad']).max()) > 0


def check_perturbed_nrm_grad(dev):
    """perturbed_nrm_grad against its restatement: a normal map that varies (a constant one gives exactly zero)"""
    base, ex, mvp, cam, draws = scene(dev)
    g = torch.Generator().manual_seed(29)
    with torch.no_grad():
        ex.material['normal'].data.copy_((torch.tensor([0.0, 0.0, 1.0]) + 0.4 * torch.randn(1, TEX, TEX, 3, generator=g)).to(dev))
        out = render(ex, None, mvp, cam, draws, _keep_rast=True)
        rast = out['_rast'].cpu()
        ins = interior(rast)
        E = _ex_np(ex)
        maps = [ex.material[k].data.detach().cpu() for k in ('kd', 'ks')]
        nm = ex.material['normal'].data.detach().cpu()
        y = {dt: _y_buffers(E, rast, None, [m.to(dt) for m in maps], nm.to(dt), draws, cam.cpu(), dt) for dt in (torch.float64, torch.float32)}
        assert float(y[torch.float64]['perturbed_nrm_grad'][ins].max()) > 1e-3
        for k in ('perturbed_nrm', 'perturbed_nrm_grad', 'normal'):
            assert_close(f'{k}, random normal map, interior', out[k][..., :3].cpu()[ins], y[torch.float64][k][ins], y[torch.float32][k][ins])


def _loss_weights(ins):
    g = torch.Generator().manual_seed(41)
    w = torch.rand(2, B, H, W, 3, generator=g, dtype=torch.float64) + 0.5
    return w * ins[None, ..., None]


def check_branch_gradients(dev, fused):
    """d(loss on shaded + normal) / d(kd, ks, normal maps) against float64 autograd of the restatement (ks enters through nothing in this loss: its
    gradient is checked through a ks term added to the loss)"""
    base, ex, mvp, cam, draws = scene(dev, tilt=TILT)
    names = ('kd', 'ks', 'normal')
    (out, n) = routes_taken(lambda: render(ex, None, mvp, cam, draws, fused=fused, buffers=('shaded', 'normal', 'ks', '_rast')))
    assert n == ({'fused': 1, 'composed': 0} if fused else {'fused': 0, 'composed': 1}), n
    rast = out['_rast'].detach().cpu()
    ins = interior(rast)
    w = _loss_weights(ins)
    wd = w.float().to(dev)
    loss = (out['shaded'][..., :3] * wd[0]).sum() + (out['normal'][..., :3] * wd[1]).sum() + (out['ks'][..., :3] * wd[1]).sum()
    loss.backward()
    E = _ex_np(ex)
    ref = {}
    for dt in (torch.float64, torch.float32):
        ms = [ex.material[k].data.detach().cpu().to(dt).requires_grad_(True) for k in names]
        y = _y_buffers(E, rast, None, ms[:2], ms[2], draws, cam.cpu(), dt)
        ((y['shaded'] * w[0].to(dt)).sum() + (y['normal'] * w[1].to(dt)).sum() + (y['ks'] * w[1].to(dt)).sum()).backward()
        ref[dt] = [m.grad for m in ms]
    for i, k in enumerate(names):
        got = ex.material[k].data.grad
        assert got is not None and float(got.abs().sum()) > 0, f'no gradient reaches the {k} map'
        assert_close(f"d loss / d {k} map [{'fused' if fused else 'composed'}] vs float64 autograd", got, ref[torch.float64][i], ref[torch.float32][i])


def check_position_gradient(dev):
    """v_pos requires grad: the composed route is taken whatever D3H_TEXMAT_FUSED says, and d loss / d v_pos matches the restatement in which the
    barycentrics are a function of the clip positions"""
    from render import mesh as rmesh
    base, ex, mvp, cam, draws = scene(dev, tilt=TILT)
    pos = ex.v_pos.detach().clone().requires_grad_(True)
    m = rmesh.Mesh(pos, base=ex)
    (out, n) = routes_taken(lambda: render(m, None, mvp, cam, draws, fused=True, buffers=('shaded', 'normal', '_rast')))
    assert n == {'fused': 0, 'composed': 1}, n
    rast = out['_rast'].detach().cpu()
    ins = interior(rast)
    w = _loss_weights(ins)
    wd = w.float().to(dev)
    ((out['shaded'][..., :3] * wd[0]).sum() + (out['normal'][..., :3] * wd[1]).sum()).backward()
    E = _ex_np(ex)
    ref = {}
    for dt in (torch.float64, torch.float32):
        p = ex.v_pos.detach().cpu().to(dt).requires_grad_(True)
        clip = torch.matmul(torch.nn.functional.pad(p, (0, 1), value=1.0)[None], mvp.cpu().to(dt).transpose(1, 2))
        ms = [ex.material[k].data.detach().cpu().to(dt).requires_grad_(True) for k in ('kd', 'ks', 'normal')]
        y = _y_buffers(E, rast, clip, ms[:2], ms[2], draws, cam.cpu(), dt, v_pos=p)
        ((y['shaded'] * w[0].to(dt)).sum() + (y['normal'] * w[1].to(dt)).sum()).backward()
        ref[dt] = [p.grad] + [x.grad for x in ms]
    assert float(ref[torch.float64][0].abs().max()) > 0
    assert_close('d loss / d v_pos [composed] vs float64 autograd', pos.grad, ref[torch.float64][0], ref[torch.float32][0])
    assert_close('d loss / d kd map, same render', ex.material['kd'].data.grad, ref[torch.float64][1], ref[torch.float32][1])
    assert_close('d loss / d normal map, same render', ex.material['normal'].data.grad, ref[torch.float64][3], ref[torch.float32][3])


def check_branch_options(dev):
    base, ex, mvp, cam, draws = scene(dev)
    with torch.no_grad():
        full = render(ex, None, mvp, cam, draws)
        only = render(ex, None, mvp, cam, draws, buffers=('shaded',))
        assert _public(only) == ['shaded'] and torch.equal(only['shaded'], full['shaded'])
    live = render(ex, None, mvp, cam, draws, _grad_buffers=('shaded',))
    assert live['shaded'].requires_grad and not live['kd_grad'].requires_grad and not live['normal'].requires_grad
    assert set(live['_layout']) == {'shaded'} and live['_stacked'].shape[-1] == 4
    with torch.no_grad():
        ms = render(ex, None, mvp, cam, None, spp=2, msaa=True)
        assert ms['kd'].shape == (B, H, W, 4) and bool(torch.isfinite(ms['kd']).all()) and float(ms['kd'][..., 3].max()) == 1.0
        ss = render(ex, None, mvp, cam, None, spp=2)
        assert ss['kd'].shape == (B, H, W, 4) and bool(torch.isfinite(ss['normal']).all())
    from render import mesh as rmesh, texture as RT
    with pytest.raises(NotImplementedError, match='transparency'):
        four = rmesh.Mesh(base=ex)
        four.material = dict(ex.material, kd=RT.Texture2D(torch.ones(1, 4, 4, 4, device=dev)))
        render(four, None, mvp, cam, draws)
    with pytest.raises(ValueError, match='v_tex'):
        bare = rmesh.Mesh(base=ex)
        bare.v_tex = None
        render(bare, None, mvp, cam, draws)


# ---- 5. round trip -----------------------------------------------------------------------------------------------------------------------
def check_round_trip(dev, tmp_path):
    from d3h import export
    from render import obj, util
    base, ex, mvp, cam, draws = scene(dev)
    with torch.no_grad():
        # colours a PNG can hold: the position moved into [0.1, 0.9]
        ex.material['kd'].data.copy_(ex.material['kd'].data * 0.6 + 0.5)
        ex.material['ks'].data.copy_(ex.material['ks'].data * 0.6 + 0.5)
        obj.write_obj(str(tmp_path), ex)
        back = export.load_textured_mesh(os.path.join(str(tmp_path), 'mesh.obj'), device=dev)
        assert back.material['filter_mode'] == 'linear' and back.v_tng is not None and back.t_tng_idx is back.t_nrm_idx
        assert torch.equal(back.t_pos_idx, ex.t_pos_idx) and torch.equal(back.t_tex_idx, ex.t_tex_idx) and back.material['kd'].data.shape == (1, TEX, TEX, 3)
        a = render(ex, None, mvp, cam, draws, buffers=('kd', 'ks'))
        b = render(back, None, mvp, cam, draws, buffers=('kd', 'ks'))
        # kd is stored as 8-bit sRGB: rounding moves the sRGB value by at most half a step, 0.5 / 255; srgb_to_rgb is convex and increasing, so over
        # [0, 1] its steepest half step is the one that ends at 1.  A bilinear blend (weights sum to 1) and the antialias blend cannot widen it.  The uv
        # coordinates pass through text as (u, 1 - v) in float32: 2^-23 of a texture that changes by at most 1 per texel, i.e. TEX 2^-23.
        one = torch.ones(1, dtype=torch.float64)
        step = float(util.srgb_to_rgb(one) - util.srgb_to_rgb(one - 0.5 / 255))
        bound = step + TEX * 2.0 ** -23 + 1e-6
        d = float((a['kd'] - b['kd']).abs().max())
        print(f'round trip kd: off by {d:.3e} (bound {bound:.3e}: half an sRGB step at 1 is {step:.3e})')
        assert d <= bound
        ks_bound = 0.5 / 255 + TEX * 2.0 ** -23 + 1e-6                    # ks is stored linearly
        d = float((a['ks'] - b['ks']).abs().max())
        print(f'round trip ks: off by {d:.3e} (bound {ks_bound:.3e})')
        assert d <= ks_bound
        assert float((a['kd'] - b['kd']).abs().max()) > 0
        # a file without normals: auto_normals
        nn = type(ex)(base=ex)
        nn.v_nrm = None
        nn.t_nrm_idx = None
        folder = os.path.join(str(tmp_path), 'nn')
        os.makedirs(folder)
        obj.write_obj(folder, nn)
        back2 = export.load_textured_mesh(os.path.join(folder, 'mesh.obj'), filter_mode='nearest', device=dev)
        assert back2.v_nrm is not None and back2.material['filter_mode'] == 'nearest' and back2.v_tng.shape == back2.v_nrm.shape


# ---- 6. no change elsewhere --------------------------------------------------------------------------------------------------------------
def check_mlp_branch_unchanged(dev):
    """an MLP material takes the code the parent commit ran, whatever use_uv is and whatever the mesh carries: the same bits under fixed draws"""
    from render import mesh as rmesh
    base, ex, mvp, cam, draws = scene(dev)
    with torch.no_grad():
        (ref, n) = routes_taken(lambda: render(base, base, mvp, cam, draws, use_uv=False))
        assert n == {'fused': 0, 'composed': 0}
        from render import render as rr
        assert _public(ref) == sorted(rr.ALL_BUFFERS)
        carrying = rmesh.Mesh(base=ex)                     # uvs and tangents on the mesh, the MLP material: still the MLP branch
        carrying.material = base.material
        for mesh in (base, carrying):
            for use_uv in (True, False):
                for fused in (None, True, False):
                    (out, n) = routes_taken(lambda: render(mesh, base, mvp, cam, draws, use_uv=use_uv, fused=fused))
                    assert n == {'fused': 0, 'composed': 0}
                    assert _public(out) == _public(ref)
                    for k in _public(ref):
                        assert torch.equal(out[k], ref[k]), k
                    assert torch.equal(out['visible_triangles'], ref['visible_triangles'])
    # and its gradient
    p = base.v_pos.detach().clone().requires_grad_(True)
    grads = []
    for use_uv in (True, False):
        m = rmesh.auto_normals(rmesh.Mesh(p, base.t_pos_idx, material=base.material))
        out = render(m, base, mvp, cam, draws, use_uv=use_uv, buffers=('shaded', 'normal'))
        grads.append(torch.autograd.grad(out['shaded'].sum() + (out['normal'] * 0.5).sum(), p)[0])
    if dev == 'cpu':
        assert torch.equal(grads[0], grads[1])              # (on the GPU the scatter's atomics reorder the sums from run to run)
    else:
        assert_floor('MLP branch position gradient, use_uv True vs False', grads[0], grads[1])
