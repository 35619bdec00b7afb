"""Check functions of render.optixutils and what it stands on (csrc/bvh.hip, csrc/envshade.hip, csrc/denoise.hip; d3h/raytrace.py, d3h/envshade.py,
d3h/denoise.py), shared by tests/test_optixutils_emul.py (host emulation of the kernel sources) and tests/test_gpu_optixutils.py (MI355X).  Same shapes
on both.  Every fixture is generated here from a seed.

Occlusion is exact: the yardstick is a float64 Moeller-Trumbore test over ALL triangles; rays that graze an edge or a range end (any of |u|, |v|,
|1-u-v|, |t - range end| below 1e-5 while the other conditions hold to 1e-4) are left out, and their share is capped before the code under test runs.

Parity rule for the float tensors (the project's rule, tests/renderutils_cases.py): max|got - f64| / max|f64| <= max(5 * ref32_err, 2^-20) per
tensor, f64 the yardstick in float64 and ref32_err the distance of the same yardstick code run in float32 on the CPU.  Every figure is printed
before it is asserted (run with -s).
  * shading: `shade_yardstick(dtype)` is the estimator in torch with the same PCG stream, the same permutations and brute-force visibility;
    directions, pdfs and visibility are computed without gradient, so autograd gives the gradients.  It returns the discrete decisions of every
    sample (light texel, lobe, visibility, front-facing tests); a pixel any of whose decisions differs between float64 and float32 is left out
    (at most 1 % may be).  The cotangents are zero on those pixels, for the kernels and the yardsticks alike, so d(light) is compared whole.
  * shading as an estimator: independent of that yardstick's sampling, the mean over 4096 pixels that share one g-buffer entry is held to a
    float64 quadrature of f L V over the lat-long map (16 x 16 sub-samples per texel) within 5 standard errors.
  * denoiser: the torch composition of the forward in float64 with autograd for d(col), and its float32 twin."""
import functools
import math
import zlib

import numpy as np
import torch

import render.optixutils as ou
from d3h import _lib as L, raytrace as RT, envshade as ES, denoise as DN, bsdf as DB

FLOOR = 2.0 ** -20
PI = math.pi


def rel(got, ref):
    got = got.detach().cpu().double().numpy() if torch.is_tensor(got) else np.asarray(got, np.float64)
    ref = ref.detach().cpu().double().numpy() if torch.is_tensor(ref) else np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.isfinite(got).all()
    return float(np.abs(got - ref).max() / np.abs(ref).max())


def assert_close(what, got, ref, ref32):
    ref32_err = rel(ref32, ref)
    tol = max(5.0 * ref32_err, FLOOR)
    r = rel(got, ref)
    print(f'{what:56s} {r:.3e}  (ref32_err {ref32_err:.2e}, bound {tol:.3e}, {r / tol:.2f} of it)')
    assert r <= tol, (what, r, tol)


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


# ---- occlusion ---------------------------------------------------------------------------------------------------------------------------
SOUP_F = (0, 1, 2, 3, 64, 65, 1000)
MESHES = tuple(f'soup{F}' for F in SOUP_F) + ('same_centroid', 'zero_area', 'int64')
N_RAYS = 4096
AMBIGUOUS_CAP = 0.005


def _soup(rng, F):
    """F triangles: centres uniform in [-1,1]^3, vertex offsets uniform in +-0.25"""
    v = rng.uniform(-1.0, 1.0, (F, 1, 3)) + rng.uniform(-0.25, 0.25, (F, 3, 3))
    return v.reshape(-1, 3).astype(np.float32), np.arange(3 * F).reshape(F, 3).astype(np.int32)


@functools.lru_cache(maxsize=None)
def mesh(name):
    rng = _rng('mesh ' + name)
    if name.startswith('soup'):
        return _soup(rng, int(name[4:]))
    if name == 'same_centroid':
        # 300 triangles whose vertex sums are the same float bits (dyadic offsets, o2 = -(o0 + o1)): one centroid, one Morton code, 300 keys that differ
        # in the index half only
        o = rng.integers(-16, 17, (300, 2, 3)) / 64.0
        o = np.concatenate([o, -o.sum(1, keepdims=True)], 1)
        v = np.array([0.25, -0.5, 0.125]) + o
        return v.reshape(-1, 3).astype(np.float32), np.arange(900).reshape(300, 3).astype(np.int32)
    if name == 'zero_area':
        # an indexed mesh: 200 triangles over 150 shared vertices, 50 more with a repeated vertex (an edge or a point), shuffled among them
        verts = rng.uniform(-1.0, 1.0, (150, 3)).astype(np.float32)
        tris = np.stack([rng.permutation(150)[:3] for _ in range(200)])
        i, j = rng.integers(0, 150, 50), rng.integers(0, 150, 50)
        flat = np.stack([i, j, np.where(np.arange(50) % 2 == 0, j, i)], 1)
        flat[::5] = flat[::5, :1]
        tris = np.concatenate([tris, flat])[rng.permutation(250)]
        return verts, tris.astype(np.int32)
    if name == 'int64':
        verts = rng.uniform(-1.0, 1.0, (80, 3)).astype(np.float32)
        return verts, np.stack([rng.permutation(80)[:3] for _ in range(100)]).astype(np.int64)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def rays(name):
    """4096 rays: a quarter random, a quarter axis-parallel (two direction components exactly zero), half aimed from a random origin at a uniformly
    drawn interior point of a random triangle (t = 1 there)"""
    verts, tris = mesh(name)
    rng = _rng('rays ' + name)
    N, q = N_RAYS, N_RAYS // 4
    org = rng.uniform(-2.0, 2.0, (N, 3))
    d = rng.standard_normal((N, 3))
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    org[q:2 * q] = rng.uniform(-1.5, 1.5, (q, 3))
    d[q:2 * q] = 0.0
    d[q + np.arange(q), rng.integers(0, 3, q)] = rng.choice([-1.0, 1.0], q)
    if len(tris):
        proper = np.nonzero((tris[:, 0] != tris[:, 1]) & (tris[:, 1] != tris[:, 2]) & (tris[:, 0] != tris[:, 2]))[0]     # not at a collapsed triangle: its
        f = proper[rng.integers(0, len(proper), N - 2 * q)]                                                           # points are vertices and edges of others
        b = rng.dirichlet((1.0, 1.0, 1.0), N - 2 * q)
        target = (b[:, :, None] * verts.astype(np.float64)[tris[f].astype(np.int64)]).sum(1)
        d[2 * q:] = target - org[2 * q:]
    return org.astype(np.float32), d.astype(np.float32)


def brute(verts, tris, org, dirs, tmin=0.0, tmax=1e16, dt=np.float64):
    """-> (occluded [N], ambiguous [N], distance of the first hit [N] (inf = none)): Moeller-Trumbore over all triangles of non-zero area"""
    N = len(org)
    hit, amb, first = np.zeros(N, bool), np.zeros(N, bool), np.full(N, np.inf)
    if len(tris) == 0 or len(verts) == 0:
        return hit, amb, first
    v = verts.astype(dt)[tris.astype(np.int64)]
    v0, e1, e2 = v[:, 0], v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
    nrm = np.cross(e1, e2)
    live = (nrm * nrm).sum(-1) > 0                              # a repeated vertex makes the cross product exactly zero
    v0, e1, e2 = v0[None, live], e1[None, live], e2[None, live]
    for s in range(0, N, 512):
        o, d = org[s:s + 512].astype(dt)[:, None], dirs[s:s + 512].astype(dt)[:, None]
        with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
            p = np.cross(d, e2)
            det = (e1 * p).sum(-1)
            inv = 1.0 / det
            tv = o - v0
            u = (tv * p).sum(-1) * inv
            qv = np.cross(tv, e1)
            w = (d * qv).sum(-1) * inv
            t = (e2 * qv).sum(-1) * inv
            quant = [u, w, 1.0 - u - w, t - dt(tmin), dt(tmax) - t]
            ok = det != 0
            h = ok & np.all([c >= 0 for c in quant], 0)
            a = np.zeros_like(h)
            for k in range(5):
                a |= (np.abs(quant[k]) < 1e-5) & np.all([quant[j] >= -1e-4 for j in range(5) if j != k], 0)
        hit[s:s + 512] = h.any(1)
        amb[s:s + 512] = (a & ok).any(1)
        first[s:s + 512] = np.where(h, t, np.inf).min(1)
    return hit, amb, first


@functools.lru_cache(maxsize=None)
def occlusion_reference(name, tmin=0.0, tmax=1e16):
    verts, tris = mesh(name)
    org, d = rays(name)
    return brute(verts, tris, org, d, tmin, tmax)


def _build(dev, name):
    verts, tris = mesh(name)
    return RT.Bvh(torch.from_numpy(verts).to(dev), torch.from_numpy(tris).to(dev))


def _compare_occlusion(what, got, ref):
    hit, amb, _ = ref
    share = float(amb.mean())
    print(f'{what}: {int(hit.sum())} of {len(hit)} rays occluded, {int(amb.sum())} ambiguous (left out)')
    assert share <= AMBIGUOUS_CAP, (what, share)
    return hit, ~amb


def check_occlusion(dev, name):
    org, d = rays(name)
    ref = occlusion_reference(name)
    hit, keep = _compare_occlusion(name, None, ref)             # the cap on the excluded share, before the code under test is looked at
    if name not in ('soup0',):
        assert hit.mean() > (0.2 if name != 'soup1' else 0.1), 'the aimed rays no longer hit'
    got = _build(dev, name).occluded(torch.from_numpy(org).to(dev), torch.from_numpy(d).to(dev))
    assert got.dtype == torch.bool and tuple(got.shape) == (N_RAYS,)
    got = got.cpu().numpy()
    bad = np.nonzero((got != hit) & keep)[0]
    print(f'{name}: {len(bad)} rays differ from the float64 test over all triangles' + (f', first {bad[:8]}' if len(bad) else ''))
    assert len(bad) == 0


def check_occlusion_range(dev, name='soup1000'):
    """tmax, then tmin, set to the median hit distance (as the float32 the kernel receives); a batch shape of more than one dim"""
    org, d = rays(name)
    hit, _, first = occlusion_reference(name)
    mid = float(np.float32(np.median(first[hit])))
    bvh = _build(dev, name)
    o, dd = torch.from_numpy(org).to(dev).reshape(8, 512, 3), torch.from_numpy(d).to(dev).reshape(8, 512, 3)
    for what, kw in (('tmax', dict(tmax=mid)), ('tmin', dict(tmin=mid))):
        ref = occlusion_reference(name, **kw)
        h, keep = _compare_occlusion(f'{name}, {what} = {mid:.4f}', None, ref)
        assert 0.05 < h.mean() < hit.mean(), 'the range no longer cuts hits away'
        got = bvh.occluded(o, dd, **kw)
        assert tuple(got.shape) == (8, 512)
        bad = int(((got.reshape(-1).cpu().numpy() != h) & keep).sum())
        print(f'{name}, {what}: {bad} rays differ')
        assert bad == 0


def check_occlusion_validation(dev):
    import pytest
    bvh = _build(dev, 'soup3')
    with pytest.raises(RuntimeError):
        bvh.occluded(torch.zeros(4, 3, device=dev), torch.zeros(5, 3, device=dev))
    with pytest.raises(RuntimeError):
        RT.Bvh(torch.zeros(4, 3, device=dev), torch.zeros(2, 3, device=dev))            # float indices
    empty_v = RT.Bvh(torch.zeros(0, 3, device=dev), torch.zeros(2, 3, dtype=torch.int32, device=dev))      # V = 0: an empty scene
    assert not empty_v.occluded(torch.zeros(7, 3, device=dev), torch.ones(7, 3, device=dev)).any()


# ---- shading: the yardstick ---------------------------------------------------------------------------------------------------------------
ONE_BELOW = float(np.float32(0.99999994))
MIN_ROUGHNESS = 0.08
BSDFS = ('pbr', 'diffuse', 'white')


def _pcg(state):
    word = ((state >> ((state >> np.uint32(28)) + np.uint32(4))) ^ state) * np.uint32(277803737)
    return (word >> np.uint32(22)) ^ word, state * np.uint32(747796405) + np.uint32(2891336453)


def sample_stream(seed, npix, perms, n):
    """the reference's draws as float32: [npix, n^2, 5] = (light sx, sy, bsdf sx, sy, sz) -- these values are the definition, bit for bit"""
    with np.errstate(over='ignore'):
        g, _ = _pcg(np.full(1, seed & 0xffffffff, np.uint32))
        s, _ = _pcg(np.arange(npix, dtype=np.uint32))
        state = g ^ s
        R = np.uint32(perms.shape[0])
        r, state = _pcg(state)
        li = (r % R).astype(np.int64)
        r, state = _pcg(state)
        bi = (r % R).astype(np.int64)
        strata = np.float32(1.0) / np.float32(n)
        out = np.zeros((npix, n * n, 5), np.float32)

        def uni():
            nonlocal state
            r, state = _pcg(state)
            return (r & np.uint32(0xFFFFFF)).astype(np.float32) / np.float32(0x1000000)
        for k in range(n * n):
            out[:, k, 0] = ((perms[li, k] % n).astype(np.float32) + uni()) * strata
            out[:, k, 1] = ((perms[li, k] // n).astype(np.float32) + uni()) * strata
            out[:, k, 2] = ((perms[bi, k] % n).astype(np.float32) + uni()) * strata
            out[:, k, 3] = ((perms[bi, k] // n).astype(np.float32) + uni()) * strata
            out[:, k, 4] = uni()
    assert out.dtype == np.float32
    return out


def _dot(a, b):
    return (a * b).sum(-1, keepdim=True)


def _unit0(v):
    l = v.norm(dim=-1, keepdim=True)
    return torch.where(l > 0, v / torch.where(l > 0, l, torch.ones_like(l)), torch.zeros_like(v))


def _onb(n):
    x, y, z = n[..., 0:1], n[..., 1:2], n[..., 2:3]
    sign = torch.where(z >= 0, torch.ones_like(z), -torch.ones_like(z))
    a = -1.0 / (sign + z)
    b = x * y * a
    return torch.cat([1.0 + sign * x * x * a, sign * b, -sign * x], -1), torch.cat([b, sign + y * y * a, -y], -1)


def _local(v, U, V, W):
    return torch.cat([_dot(v, U), _dot(v, V), _dot(v, W)], -1)


def _dir_to_tc(d):
    u = torch.atan2(d[..., 0], -d[..., 2]) / (2.0 * PI) + 0.5
    v = torch.acos(d[..., 1].clamp(-1.0, 1.0)) / PI
    return u, v


def _texel(c, size):
    return (c * size).to(torch.int64).clamp(0, size - 1)


def _sample_cdf(cdf, x):
    """cdf [P, size], x [P] -> (index [P], position inside the entry [P])"""
    x = x.clamp(max=ONE_BELOW)
    size = cdf.shape[-1]
    idx = torch.searchsorted(cdf.contiguous(), x[:, None].contiguous(), right=True)[:, 0].clamp(max=size - 1)
    at = cdf.gather(1, idx[:, None])[:, 0]
    below = torch.where(idx > 0, cdf.gather(1, (idx - 1).clamp(min=0)[:, None])[:, 0], torch.zeros_like(at))
    return idx, ((x - below) / (at - below)).clamp(max=ONE_BELOW)


def _luminance(c):
    return c[..., 0:1] * 0.2126 + c[..., 1:2] * 0.7152 + c[..., 2:3] * 0.0722


def _g1(a2, c):
    c2 = c * c
    return torch.where(c > 0, 2.0 / (1.0 + torch.sqrt(1.0 + a2 * ((1.0 - c2).clamp(min=0.0) / c2))), torch.zeros_like(c))


def _ndf(alpha, c):
    a2 = alpha * alpha
    d = (c * a2 - c) * c + 1.0
    return a2 / (d * d * PI)


def _vndf_pdf(alpha, wo_l, h):
    woH = _dot(wo_l, h)
    return _g1(alpha * alpha, wo_l[..., 2:3]) * _ndf(alpha, h[..., 2:3]) * woH.clamp(min=0.0) / wo_l[..., 2:3] / (4.0 * woH)


def _ggx_pdf(N, wo, wi, alpha):
    W = _unit0(N)
    U, V = _onb(W)
    wo_l, wi_l = _local(wo, U, V, W), _local(wi, U, V, W)
    ok = (wo_l[..., 2:3] > 0) & (wi_l[..., 2:3] > 0)
    return torch.where(ok, _vndf_pdf(alpha, wo_l, _unit0(wi_l + wo_l)), torch.zeros_like(alpha)), ok


def _ggx_sample(N, wo, ux, uy, alpha):
    W = _unit0(N)
    U, V = _onb(W)
    wo_l = _unit0(_local(wo, U, V, W))
    ok = wo_l[..., 2:3] > 0
    Vh = _unit0(torch.cat([alpha * wo_l[..., 0:1], alpha * wo_l[..., 1:2], wo_l[..., 2:3]], -1))
    z = torch.zeros_like(Vh)
    z[..., 2] = 1.0
    x1 = torch.zeros_like(Vh)
    x1[..., 0] = 1.0
    T1 = torch.where(Vh[..., 2:3] < 0.9999, _unit0(torch.cross(z, Vh, dim=-1)), x1)
    T2 = torch.cross(Vh, T1, dim=-1)
    r, phi = torch.sqrt(ux), (2.0 * PI) * uy
    t1, t2, s = r * torch.cos(phi), r * torch.sin(phi), 0.5 * (1.0 + Vh[..., 2:3])
    t2 = (1.0 - s) * torch.sqrt(1.0 - t1 * t1) + s * t2
    Nh = T1 * t1 + T2 * t2 + Vh * torch.sqrt((1.0 - t1 * t1 - t2 * t2).clamp(min=0.0))
    h = _unit0(torch.cat([alpha * Nh[..., 0:1], alpha * Nh[..., 1:2], Nh[..., 2:3].clamp(min=0.0)], -1))
    pdf = _vndf_pdf(alpha, wo_l, h)
    wi_l = h * (_dot(wo_l, h) * 2.0) - wo_l
    wi = _unit0(U * wi_l[..., 0:1] + V * wi_l[..., 1:2] + W * wi_l[..., 2:3])
    return torch.where(ok, wi, torch.zeros_like(wi)), torch.where(ok, pdf, torch.zeros_like(pdf))


def _cosine_sample(N, u, v):
    W = _unit0(N)
    U, V = _onb(W)
    phi, ct, st = 2.0 * PI * u, torch.sqrt(v), torch.sqrt(1.0 - v)
    return _unit0(U * (torch.cos(phi) * st) + V * (torch.sin(phi) * st) + W * ct), (ct / PI).clamp(min=0.000001)


def _add_pdf(pdf, other, weight):
    return pdf + torch.where(weight > 0.000001, other * weight, torch.zeros_like(pdf))


def _tri_hit(tri, o, d, tmin=0.0, tmax=1e16):
    """tri [F,3,3], o, d [P,3] -> any hit [P] (two-sided Moeller-Trumbore in the tensors' dtype)"""
    if tri.shape[0] == 0:
        return torch.zeros(o.shape[0], dtype=torch.bool)
    v0, e1, e2 = tri[None, :, 0], tri[None, :, 1] - tri[None, :, 0], tri[None, :, 2] - tri[None, :, 0]
    o, d = o[:, None], d[:, None].expand(-1, tri.shape[0], -1)
    p = torch.cross(d, e2.expand_as(d), dim=-1)
    det = (e1 * p).sum(-1)
    inv = 1.0 / det
    tv = o - v0
    u = (tv * p).sum(-1) * inv
    q = torch.cross(tv, e1.expand_as(tv), dim=-1)
    v = (d * q).sum(-1) * inv
    t = (e2 * q).sum(-1) * inv
    return ((det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t >= tmin) & (t <= tmax)).any(1)


def shade_yardstick(fx, dtype, BSDF, n, seed, shadow_scale, g_diff=None, g_spec=None):
    """-> dict: diff, spec [P,3]; with cotangents also d_pos, d_nrm, d_kd, d_ks [P,3] and d_light; decisions [P, 2 n^2, 6] int64"""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
    P = fx['mask'].size
    mode = BSDFS.index(BSDF)
    mask = torch.from_numpy(fx['mask'].reshape(-1) > 0)
    leaf = {k: t(fx[k]).reshape(P, 3).requires_grad_(g_diff is not None) for k in ('pos', 'nrm', 'kd', 'ks')}
    light = t(fx['light']).requires_grad_(g_diff is not None)
    pos, nrm, kd, ks = leaf['pos'], leaf['nrm'], leaf['kd'], leaf['ks']
    ro, view = t(fx['ro']).reshape(P, 3), t(fx['view']).reshape(P, 3)
    pdf, rows, cols = t(fx['pdf']), t(fx['rows']), t(fx['cols'])
    tri = t(fx['verts'])[torch.from_numpy(fx['tris'].astype(np.int64))] if len(fx['tris']) else torch.zeros(0, 3, 3, dtype=dtype)
    PH, PW = pdf.shape
    LH, LW = light.shape[:2]
    draws = t(sample_stream(seed, P, fx['perms'], n))                      # float32 values, exact in either dtype

    def light_pdf(d):
        u, v = _dir_to_tc(d)
        w = PH * PW / (2.0 * PI * PI * torch.sin(v * PI).clamp(min=0.0001))
        return (pdf[_texel(v, PH), _texel(u, PW)] * w)[:, None]

    with torch.no_grad():
        alpha = (ks[:, 1:2] * ks[:, 1:2]).detach()
        wo = _unit0(view - pos)
        metal = ks[:, 2:3]
        kb = 0.04 * (1.0 - metal) + kd * metal
        wd = (1.0 - metal) * _luminance(kd)
        W = _unit0(nrm)
        U, V = _onb(W)
        c = _unit0(_local(wo, U, V, W))[:, 2:3]
        s = (1.0 - c.clamp(1e-4, 1.0 - 1e-4)) ** 5.0
        ws = torch.where(c > 0, _luminance(kb * (1.0 - s) + s), torch.zeros_like(c))
        pD = torch.where(wd + ws > 0, wd / (wd + ws), torch.ones_like(wd))
        pS = 1.0 - pD

        def bsdf_pdf(wi):
            below = torch.minimum(_dot(nrm, wo), _dot(nrm, wi)) < 1e-6
            gp, _ = _ggx_pdf(nrm, wo, wi, alpha)
            p = torch.zeros_like(alpha)
            p = torch.where(pD > 0, _add_pdf(p, _dot(nrm, wi).clamp(min=0.0) / PI, pD), p)
            p = torch.where(pS > 0, _add_pdf(p, gp, 1.0 - pD), p)
            return torch.where(below, torch.ones_like(p), p), below

        samples = []                                        # (wi, pdf_light + pdf_bsdf, lobe)
        for k in range(n * n):
            y, ry = _sample_cdf(rows[None].expand(P, -1), draws[:, k, 1])
            x, rx = _sample_cdf(cols[y], draws[:, k, 0])
            phi, theta = ((x + rx) / PW * 2.0 - 1.0) * PI, (y + ry) / PH * PI
            st = torch.sin(theta)
            wi = torch.stack([st * torch.sin(phi), torch.cos(theta), -st * torch.cos(phi)], -1)
            pb, below = bsdf_pdf(wi)
            samples.append((wi, light_pdf(wi) + pb, torch.zeros(P, dtype=torch.int64), below[:, 0]))
            lobe = draws[:, k, 4:5] < pD
            wc, pc = _cosine_sample(nrm, draws[:, k, 2:3], draws[:, k, 3:4])
            gp, _ = _ggx_pdf(nrm, wo, wc, alpha)
            pc = pc * pD
            pc = torch.where(pS > 0, _add_pdf(pc, gp, 1.0 - pD), pc)
            tiny = pD < 0.0001
            wc, pc = torch.where(tiny, nrm.detach(), wc), torch.where(tiny, torch.ones_like(pc), pc)
            wg, pg = _ggx_sample(nrm, wo, draws[:, k, 2:3], draws[:, k, 3:4], alpha)
            pg = pg * (1.0 - pD)
            pg = torch.where(pD > 0, _add_pdf(pg, _dot(nrm, wg).clamp(min=0.0) / PI, pD), pg)
            wi, pb = torch.where(lobe, wc, wg), torch.where(lobe, pc, pg)
            samples.append((wi, light_pdf(wi) + pb, 1 + lobe[:, 0].to(torch.int64), torch.zeros(P, dtype=torch.bool)))

    frac = 1.0 / (n * n)
    wo_g = torch.nn.functional.normalize(view - pos, dim=-1)
    kb_g = 0.04 * (1.0 - ks[:, 2:3]) + kd * ks[:, 2:3]
    diff = torch.zeros(P, 3, dtype=dtype)
    spec = torch.zeros(P, 3, dtype=dtype)
    decisions = []
    for wi, pdf_sum, lobe, below in samples:
        wi = wi.detach()
        with torch.no_grad():
            u, v = _dir_to_tc(wi)
            ty, tx = _texel(v, LH), _texel(u, LW)
            hit = _tri_hit(tri, ro, wi)
            wgt = torch.where(hit, 1.0 - shadow_scale, 1.0).to(dtype)[:, None] / pdf_sum.clamp(min=0.0001) * frac
            nwi, nwo = _dot(nrm, wi)[:, 0], _dot(nrm, wo)[:, 0]
            decisions.append(torch.stack([ty * LW + tx, lobe, hit.to(torch.int64), (nwi > 0).to(torch.int64),
                                          ((nwi > 1e-4) & (nwo > 1e-4)).to(torch.int64), below.to(torch.int64)], -1))
        Lc = light[ty, tx]
        diff = diff + DB.py_lambert(nrm, wi) * Lc * wgt
        if mode == 0:
            spec = spec + DB.py_pbr_specular(kb_g * (1.0 - ks[:, 0:1]), nrm, wo_g, wi, ks[:, 1:2] * ks[:, 1:2], MIN_ROUGHNESS) * Lc * wgt
    m = mask[:, None].to(dtype)
    diff, spec = diff * m, spec * m
    out = {'diff': diff.detach(), 'spec': spec.detach(), 'decisions': torch.stack(decisions, 1)}
    if g_diff is not None:
        ((diff * t(g_diff).reshape(P, 3)).sum() + (spec * t(g_spec).reshape(P, 3)).sum()).backward()
        for k in ('pos', 'nrm', 'kd', 'ks'):
            out['d_' + k] = leaf[k].grad if leaf[k].grad is not None else torch.zeros(P, 3, dtype=dtype)
        out['d_light'] = light.grad if light.grad is not None else torch.zeros_like(light)
    return out


# ---- shading: fixtures --------------------------------------------------------------------------------------------------------------------
def light_tables(light):
    """pdf, rows [H,W], cols [H,W] of a lat-long map as the reference's EnvironmentLight.update_pdf makes them (render/light.py:46-59), float32"""
    base = torch.from_numpy(light)
    H, W = base.shape[:2]
    Y = ((torch.arange(H, dtype=torch.float32) + 0.5) / H)[:, None].expand(H, W)
    pdf = base.max(dim=-1)[0] * torch.sin(Y * np.pi)
    pdf = pdf / pdf.sum()
    cols = torch.cumsum(pdf, dim=1)
    rows = torch.cumsum(cols[:, -1:].repeat([1, W]), dim=0)
    cols = cols / torch.where(cols[:, -1:] > 0, cols[:, -1:], torch.ones_like(cols))
    rows = rows / torch.where(rows[-1:, :] > 0, rows[-1:, :], torch.ones_like(rows))
    return pdf.numpy(), rows.numpy(), cols.numpy()


def scene_mesh(occluder=True):
    """a ground quad at y = 0 and, above it, a smaller occluder quad at y = 0.5"""
    def quad(h, y):
        return [[-h, y, -h], [h, y, -h], [h, y, h], [-h, y, h]]
    verts = quad(2.0, 0.0) + (quad(0.6, 0.5) if occluder else [])
    tris = [[0, 1, 2], [0, 2, 3]] + ([[4, 5, 6], [4, 6, 7]] if occluder else [])
    return np.array(verts, np.float32), np.array(tris, np.int32)


@functools.lru_cache(maxsize=None)
def shade_fixture(n, rough_lo=0.3, rough_hi=0.9, seed=11):
    rng = np.random.default_rng(seed + 100 * n)
    B, H, W = 2, 9, 13
    f32 = lambda a: np.ascontiguousarray(a, np.float32)
    pos = np.zeros((B, H, W, 3))
    pos[..., 0], pos[..., 2] = rng.uniform(-1.5, 1.5, (B, H, W)), rng.uniform(-1.5, 1.5, (B, H, W))
    nrm = np.array([0.0, 1.0, 0.0]) + rng.uniform(-0.3, 0.3, (B, H, W, 3))
    nrm /= np.linalg.norm(nrm, axis=-1, keepdims=True)
    view = np.broadcast_to(np.array([[0.0, 3.0, 4.0], [3.0, 2.0, -1.0]])[:, None, None, :], (B, H, W, 3))
    ks = np.stack([rng.uniform(0.0, 0.5, (B, H, W)), rng.uniform(rough_lo, rough_hi, (B, H, W)), rng.uniform(0.0, 1.0, (B, H, W))], -1)
    light = f32(rng.uniform(0.1, 4.0, (8, 16, 3)))
    pdf, rows, cols = light_tables(light)
    verts, tris = scene_mesh()
    fx = dict(mask=f32(rng.uniform(0.0, 1.0, (B, H, W)) > 0.2), pos=f32(pos), nrm=f32(nrm), view=f32(view), kd=f32(rng.uniform(0.1, 0.9, (B, H, W, 3))), ks=f32(ks),
              light=light, pdf=pdf, rows=rows[:, 0].copy(), rows2d=rows, cols=cols, verts=verts, tris=tris,
              perms=np.stack([rng.permutation(n * n) for _ in range(7)]).astype(np.int32),
              g_diff=f32(rng.standard_normal((B, H, W, 3))), g_spec=f32(rng.standard_normal((B, H, W, 3))))
    fx['ro'] = f32(fx['pos'] + np.float32(0.001) * fx['nrm'])
    return fx


SHADE_SEED = 1234567


@functools.lru_cache(maxsize=None)
def shade_reference(BSDF, n, shadow_scale):
    """-> (yardstick float64, yardstick float32, kept pixels [P] bool, cotangents zeroed on the pixels left out); asserts the 1 % cap"""
    fx = shade_fixture(n)
    dec = [shade_yardstick(fx, dt, BSDF, n, SHADE_SEED, shadow_scale)['decisions'] for dt in (torch.float64, torch.float32)]
    mask = torch.from_numpy(fx['mask'].reshape(-1) > 0)
    keep = (dec[0] == dec[1]).all(-1).all(-1) | ~mask
    out = int((~keep).sum())
    print(f'{BSDF}, n = {n}, shadow_scale {shadow_scale}: {out} of {int(mask.sum())} unmasked pixels left out (a decision differs between float64 and float32); '
          f'{float(dec[0][mask][..., 2].double().mean()):.2f} of the samples occluded')
    assert out <= 0.01 * int(mask.sum())
    k = keep.reshape(fx['mask'].shape)[..., None].numpy()
    g_diff, g_spec = fx['g_diff'] * k, fx['g_spec'] * k
    y64 = shade_yardstick(fx, torch.float64, BSDF, n, SHADE_SEED, shadow_scale, g_diff, g_spec)
    y32 = shade_yardstick(fx, torch.float32, BSDF, n, SHADE_SEED, shadow_scale, g_diff, g_spec)
    return y64, y32, keep, g_diff, g_spec


def _to(dev, a, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev).requires_grad_(grad)


def run_shade(dev, fx, BSDF, n, seed, shadow_scale, g_diff=None, g_spec=None, bwd_seed=None, strided=False, bvh=None):
    """the kernel path through d3h.envshade -> dict like shade_yardstick's"""
    bvh = bvh if bvh is not None else RT.Bvh(_to(dev, fx['verts']), _to(dev, fx['tris']))
    grad = g_diff is not None
    leaf = {k: _to(dev, fx[k], grad) for k in ('pos', 'nrm', 'kd', 'ks')}
    light = _to(dev, fx['light'], grad)
    mask, rows = _to(dev, fx['mask']), _to(dev, fx['rows'])
    if strided:         # as the reference passes them: rast[..., -1] and lgt.rows[:, 0]
        mask = torch.stack([torch.zeros_like(mask)] * 3 + [mask], -1)[..., -1]
        rows = _to(dev, fx['rows2d'])[:, 0]
        assert not mask.is_contiguous() and not rows.is_contiguous()
    diff, spec = ES.env_shade(bvh, mask, _to(dev, fx['ro']), leaf['pos'], leaf['nrm'], _to(dev, fx['view']), leaf['kd'], leaf['ks'], light, _to(dev, fx['pdf']), rows,
                              _to(dev, fx['cols']), _to(dev, fx['perms']), BSDFS.index(BSDF), n, seed, seed if bwd_seed is None else bwd_seed, shadow_scale)
    out = {'diff': diff.detach().reshape(-1, 3), 'spec': spec.detach().reshape(-1, 3)}
    if grad:
        torch.autograd.backward([diff, spec], [_to(dev, g_diff), _to(dev, g_spec)])
        for k in ('pos', 'nrm', 'kd', 'ks'):
            out['d_' + k] = None if leaf[k].grad is None else leaf[k].grad.reshape(-1, 3)
        out['d_light'] = light.grad
    return out


def check_shade_parity(dev, BSDF, n, shadow_scale):
    fx = shade_fixture(n)
    y64, y32, keep, g_diff, g_spec = shade_reference(BSDF, n, shadow_scale)
    got = run_shade(dev, fx, BSDF, n, SHADE_SEED, shadow_scale, g_diff, g_spec)
    masked = torch.from_numpy(fx['mask'].reshape(-1) <= 0)
    assert int(masked.sum()) >= 20 and (BSDF != 'pbr' or float(y64['spec'].abs().max()) > 1e-3)
    for k in ('diff', 'spec', 'd_pos', 'd_nrm', 'd_kd', 'd_ks'):
        if got[k] is None or (BSDF != 'pbr' and k != 'diff' and k != 'd_nrm'):
            # the Lambert modes: no specular, and gb_pos / gb_kd / gb_ks get None or zeros -- as the yardstick's autograd says
            assert float(y64[k].abs().max()) == 0.0
            assert got[k] is None or float(got[k].abs().max()) == 0.0, k
            continue
        assert got[k].dtype == torch.float32
        assert (got[k].cpu()[masked] == 0).all(), f'{k}: masked pixels must be exactly zero'
        assert_close(f'{BSDF} n={n} s={shadow_scale}: {k}', got[k].cpu()[keep], y64[k][keep], y32[k][keep])
    assert_close(f'{BSDF} n={n} s={shadow_scale}: d_light (whole)', got['d_light'], y64['d_light'], y32['d_light'])


def check_shade_layouts_and_seeds(dev):
    fx = shade_fixture(3)
    bvh = RT.Bvh(_to(dev, fx['verts']), _to(dev, fx['tris']))
    run = lambda **kw: run_shade(dev, fx, 'pbr', 3, kw.pop('seed', SHADE_SEED), 1.0, fx['g_diff'], fx['g_spec'], bvh=bvh, **kw)
    a, b, c, d = run(), run(strided=True), run(), run(seed=SHADE_SEED + 1)
    for k in ('diff', 'spec', 'd_pos', 'd_nrm', 'd_kd', 'd_ks'):
        assert torch.equal(a[k], b[k]), f'{k}: a non-contiguous mask / rows changed the result'
        assert torch.equal(a[k], c[k]), f'{k}: the same seed gave another result'
        assert not torch.equal(a[k], d[k]), f'{k}: another seed gave the same result'
    # d_light is summed with float atomics: equal up to their order
    assert_close('d_light, strided against contiguous inputs', b['d_light'], a['d_light'].double(), c['d_light'])
    # a backward seed of its own: the forward is that of the forward seed, the gradients those of a run whose seed is the backward's
    e = run(bwd_seed=SHADE_SEED + 1)
    assert torch.equal(e['diff'], a['diff']) and torch.equal(e['d_nrm'], d['d_nrm']) and not torch.equal(e['d_nrm'], a['d_nrm'])


def check_shade_low_roughness(dev):
    """roughness in [0.08, 0.2]: finite, masked pixels zero (no parity claim: the GGX lobe amplifies float32 rounding there)"""
    fx = shade_fixture(3, 0.08, 0.2)
    got = run_shade(dev, fx, 'pbr', 3, SHADE_SEED, 1.0, fx['g_diff'], fx['g_spec'])
    masked = torch.from_numpy(fx['mask'].reshape(-1) <= 0)
    for k, v in got.items():
        assert torch.isfinite(v).all(), k
        if k != 'd_light':
            assert (v.cpu()[masked] == 0).all(), k
        print(f'low roughness: max |{k}| = {float(v.abs().max()):.3e}')
    assert float(got['spec'].abs().max()) > 0 and float(got['d_ks'].abs().max()) > 0


# ---- shading as an estimator -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def estimator_fixture(case):
    rng = np.random.default_rng(77)
    S = 64
    f32 = lambda a: np.ascontiguousarray(a, np.float32)
    rep = lambda v: f32(np.broadcast_to(np.asarray(v, np.float64), (1, S, S, 3)))
    nrm = np.array([0.15, 1.0, -0.1])
    nrm /= np.linalg.norm(nrm)
    light = np.ones((16, 32, 3)) if case == 'constant' else rng.uniform(0.1, 4.0, (16, 32, 3))
    light = f32(light)
    pdf, rows, cols = light_tables(light)
    verts, tris = scene_mesh() if case != 'constant' else (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    fx = dict(mask=np.ones((1, S, S), np.float32), pos=rep([0.35, 0.0, 0.25]), nrm=rep(nrm), view=rep([0.0, 3.0, 4.0]), kd=rep([0.7, 0.5, 0.3]),
              ks=rep([0.2, 0.5, 0.4]), light=light, pdf=pdf, rows=rows[:, 0].copy(), rows2d=rows, cols=cols, verts=verts, tris=tris,
              perms=np.stack([rng.permutation(16) for _ in range(64)]).astype(np.int32))
    fx['ro'] = f32(fx['pos'] + np.float32(0.001) * fx['nrm'])
    return fx


@functools.lru_cache(maxsize=None)
def quadrature(case, BSDF):
    """float64 integral over the sphere of f(wi) L(wi) V(wi), 16 x 16 midpoint sub-samples per texel -> (diff [3], spec [3])"""
    fx = estimator_fixture(case)
    dt = torch.float64
    light = torch.from_numpy(fx['light']).to(dt)
    LH, LW = light.shape[:2]
    sub = 16
    v = (torch.arange(LH * sub, dtype=dt) + 0.5) / (LH * sub)
    u = (torch.arange(LW * sub, dtype=dt) + 0.5) / (LW * sub)
    theta, phi = (v * PI)[:, None].expand(-1, LW * sub), ((u * 2.0 - 1.0) * PI)[None, :].expand(LH * sub, -1)
    st = torch.sin(theta)
    wi = torch.stack([st * torch.sin(phi), torch.cos(theta), -st * torch.cos(phi)], -1).reshape(-1, 3)
    dw = (st * (PI / (LH * sub)) * (2.0 * PI / (LW * sub))).reshape(-1, 1)
    Lc = light.repeat_interleave(sub, 0).repeat_interleave(sub, 1).reshape(-1, 3)
    one = lambda k: torch.from_numpy(fx[k][0, 0, 0].astype(np.float64))[None]
    nrm, pos, view, kd, ks, ro = one('nrm'), one('pos'), one('view'), one('kd'), one('ks'), one('ro')
    tri = torch.from_numpy(fx['verts']).to(dt)[torch.from_numpy(fx['tris'].astype(np.int64))] if len(fx['tris']) else torch.zeros(0, 3, 3, dtype=dt)
    vis = (~_tri_hit(tri, ro.expand(wi.shape[0], -1), wi)).to(dt)[:, None]
    wo = torch.nn.functional.normalize(view - pos, dim=-1)
    diff = (DB.py_lambert(nrm, wi) * Lc * vis * dw).sum(0)
    spec = torch.zeros(3, dtype=dt)
    if BSDF == 'pbr':
        kb = (0.04 * (1.0 - ks[:, 2:3]) + kd * ks[:, 2:3]) * (1.0 - ks[:, 0:1])
        spec = (DB.py_pbr_specular(kb, nrm, wo, wi, ks[:, 1:2] ** 2, MIN_ROUGHNESS) * Lc * vis * dw).sum(0)
    return diff.numpy(), spec.numpy()


def _estimate_ok(what, img, expected):
    img = img.detach().cpu().double().numpy().reshape(-1, 3)
    mean, sem = img.mean(0), img.std(0, ddof=1) / math.sqrt(img.shape[0])
    ok = True
    for c in range(3):
        print(f'{what}[{c}]: mean over {img.shape[0]} pixels {mean[c]:.5f}, quadrature {expected[c]:.5f}, |difference| {abs(mean[c] - expected[c]):.2e} against '
              f'5 standard errors = {5 * sem[c]:.2e}')
        ok &= abs(mean[c] - expected[c]) <= 5.0 * sem[c]
    return ok


@functools.lru_cache(maxsize=None)
def estimator_yardstick(case, BSDF):
    return shade_yardstick(estimator_fixture(case), torch.float64, BSDF, 4, 4242, 1.0)


def check_estimator(dev, case, BSDF):
    fx = estimator_fixture(case)
    q_diff, q_spec = quadrature(case, BSDF)
    if case == 'constant':
        print(f'constant light, no occluder: quadrature of the Lambert lobe {q_diff}')
        assert np.abs(q_diff - 1.0).max() < 1e-4
    # the yardstick first: if IT misses the quadrature, the fixture or the quadrature is wrong
    y = estimator_yardstick(case, BSDF)
    assert _estimate_ok(f'{case}/{BSDF} yardstick diff', y['diff'], q_diff)
    assert BSDF != 'pbr' or _estimate_ok(f'{case}/{BSDF} yardstick spec', y['spec'], q_spec)
    got = run_shade(dev, fx, BSDF, 4, 4242, 1.0)
    assert _estimate_ok(f'{case}/{BSDF} kernel diff', got['diff'], q_diff)
    assert BSDF != 'pbr' or (float(got['spec'].abs().max()) > 0 and _estimate_ok(f'{case}/{BSDF} kernel spec', got['spec'], q_spec))


# ---- denoiser -----------------------------------------------------------------------------------------------------------------------------
DENOISE_SHAPES = ((2, 13, 21), (1, 5, 40))
DENOISE_SIGMAS = (0.0001, 1.0, 2.0)


@functools.lru_cache(maxsize=None)
def denoise_fixture(shape):
    rng = np.random.default_rng(5 + shape[1])
    B, H, W = shape
    f32 = lambda a: np.ascontiguousarray(a, np.float32)
    nrm = np.array([0.0, 0.0, 1.0]) + rng.uniform(-0.25, 0.25, (B, H, W, 3))
    nrm[:, :, W // 2:] += np.array([0.3, 0.0, 0.0])                     # a crease
    nrm /= np.linalg.norm(nrm, axis=-1, keepdims=True)
    dz = rng.uniform(0.01, 1.0, (B, H, W))
    dz[rng.uniform(size=(B, H, W)) < 0.05] = 0.0                        # reaches the 1e-4 clamp of the depth weight
    zdz = np.stack([2.0 + rng.uniform(-0.2, 0.2, (B, H, W)), dz], -1)
    return dict(col=f32(rng.uniform(0.0, 2.0, (B, H, W, 3))), nrm=f32(nrm), zdz=f32(zdz), g=f32(rng.standard_normal((B, H, W, 4))))


def denoise_yardstick(col, nrm, zdz, sigma):
    """[B,H,W,4] in the dtype of the inputs: the forward of render/optixutils/c_src/denoising.cu as a sum over taps of shifted slices"""
    sigma = float(np.float32(sigma))
    rad = 2 * math.ceil(sigma * 2.5) + 1
    B, H, W = col.shape[:3]
    acc = torch.zeros(B, H, W, 4, dtype=col.dtype)
    one = torch.ones(B, H, W, 1, dtype=col.dtype)
    for fy in range(-rad, rad + 1):
        for fx in range(-rad, rad + 1):
            cy, cx = slice(max(0, -fy), H - max(0, fy)), slice(max(0, -fx), W - max(0, fx))          # centres whose tap is inside
            ty, tx = slice(max(0, fy), H + min(0, fy)), slice(max(0, fx), W + min(0, fx))
            if cy.stop <= cy.start or cx.stop <= cx.start:
                continue
            d2 = float(fx * fx + fy * fy)
            w = math.exp(-d2 / (2.0 * sigma * sigma)) * (nrm[:, ty, tx] * nrm[:, cy, cx]).sum(-1, keepdim=True).clamp(1e-4, 1.0) ** 128.0 * \
                torch.exp(-((zdz[:, ty, tx, 0:1] - zdz[:, cy, cx, 0:1]).abs() / (zdz[:, cy, cx, 1:2] * math.sqrt(d2)).clamp(min=1e-4)))
            part = torch.cat([col[:, ty, tx] * w, one[:, cy, cx] * w], -1)
            acc = acc + torch.nn.functional.pad(part, (0, 0, cx.start, W - cx.stop, cy.start, H - cy.stop))
    return torch.cat([acc[..., :3], acc[..., 3:].clamp(min=1e-4)], -1)


@functools.lru_cache(maxsize=None)
def denoise_reference(shape, sigma):
    fx = denoise_fixture(shape)
    res = []
    for dt in (torch.float64, torch.float32):
        col = torch.from_numpy(fx['col']).to(dt).requires_grad_(True)
        out = denoise_yardstick(col, torch.from_numpy(fx['nrm']).to(dt), torch.from_numpy(fx['zdz']).to(dt), sigma)
        out.backward(torch.from_numpy(fx['g']).to(dt))
        res.append((out.detach(), col.grad))
    return res


def check_denoiser(dev, shape, sigma):
    fx = denoise_fixture(shape)
    (o64, d64), (o32, d32) = denoise_reference(shape, sigma)
    runs = []
    for _ in range(2):
        col, nrm, zdz = _to(dev, fx['col'], True), _to(dev, fx['nrm'], True), _to(dev, fx['zdz'], True)
        out = DN.bilateral_denoise(col, nrm, zdz, sigma)
        out.backward(_to(dev, fx['g']))
        assert nrm.grad is None and zdz.grad is None
        runs.append((out.detach(), col.grad))
    out, d_col = runs[0]
    assert tuple(out.shape) == (*shape, 4) and out.dtype == torch.float32 and tuple(d_col.shape) == (*shape, 3)
    assert_close(f'denoiser {shape} sigma {sigma}: out', out, o64, o32)
    assert_close(f'denoiser {shape} sigma {sigma}: d_col', d_col, d64, d32)
    assert torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][0], runs[1][0]), 'two runs of the gather backward differ'
    shim = ou.bilateral_denoiser(_to(dev, fx['col']), _to(dev, fx['nrm']), _to(dev, fx['zdz']), sigma)
    assert torch.equal(shim, out[..., :3] / out[..., 3:])


def check_denoiser_validation(dev):
    import pytest
    z = lambda *s: torch.zeros(*s, device=dev)
    with pytest.raises(RuntimeError):
        DN.bilateral_denoise(z(1, 4, 4, 3), z(1, 4, 4, 3), z(1, 4, 4, 3), 1.0)
    with pytest.raises(RuntimeError):
        DN.bilateral_denoise(z(1, 4, 4, 3), z(1, 4, 4, 3), z(1, 4, 4, 2), 0.0)


# ---- the shim -----------------------------------------------------------------------------------------------------------------------------
def _shim_shade(dev, ctx, fx, **kw):
    rows2d = _to(dev, fx['rows2d'])
    mask = torch.stack([torch.zeros_like(_to(dev, fx['mask']))] * 3 + [_to(dev, fx['mask'])], -1)
    return ou.optix_env_shade(ctx, mask[..., -1], _to(dev, fx['ro']), _to(dev, fx['pos'], True), _to(dev, fx['nrm'], True), _to(dev, fx['view']), _to(dev, fx['kd'], True),
                              _to(dev, fx['ks'], True), _to(dev, fx['light'], True), _to(dev, fx['pdf']), rows2d[:, 0], _to(dev, fx['cols']), **kw)


def check_shim_is_lazy(dev, monkeypatch):
    """optix_build_bvh launches nothing (no library symbol is looked up, no BVH is built) until optix_env_shade or ctx.build()"""
    import pytest
    fx = shade_fixture(3)
    ctx = ou.OptiXContext()
    with pytest.raises(RuntimeError):
        _shim_shade(dev, ctx, fx, n_samples_x=2, rnd_seed=5)                 # a fresh context: nothing to trace against
    verts, tris = _to(dev, fx['verts']), _to(dev, fx['tris'])
    builds = RT.BUILDS

    def no_lib():
        raise AssertionError('optix_build_bvh reached the native library')
    with monkeypatch.context() as m:
        m.setattr(L, 'lib', no_lib)
        for _ in range(5):
            assert ou.optix_build_bvh(ctx, verts, tris, rebuild=1) is None
        assert ou.optix_build_bvh(ctx, verts[None], tris[None], rebuild=0) is None
    assert RT.BUILDS == builds and ctx.bvh is None
    shadowed = _shim_shade(dev, ctx, fx, n_samples_x=2, rnd_seed=5, BSDF='diffuse')[0]
    assert RT.BUILDS == builds + 1 and ctx.bvh is not None and ctx.bvh.F == 4
    _shim_shade(dev, ctx, fx, n_samples_x=2, rnd_seed=5, BSDF='diffuse')
    assert RT.BUILDS == builds + 1                                          # built once, used twice
    # a second optix_build_bvh before use replaces the first; an empty mesh shades as unoccluded: the bits of shadow_scale = 0
    ou.optix_build_bvh(ctx, verts, tris, rebuild=1)
    ou.optix_build_bvh(ctx, verts[:0], tris[:0], rebuild=1)
    assert RT.BUILDS == builds + 1
    open_sky = _shim_shade(dev, ctx, fx, n_samples_x=2, rnd_seed=5, BSDF='diffuse')[0]
    assert RT.BUILDS == builds + 2 and ctx.bvh.F == 0
    ctx2 = ou.OptiXContext()
    ou.optix_build_bvh(ctx2, verts, tris, rebuild=1)
    assert ctx2.build().F == 4 and RT.BUILDS == builds + 3                     # ctx.build() forces the build
    unshadowed = _shim_shade(dev, ctx2, fx, n_samples_x=2, rnd_seed=5, BSDF='diffuse', shadow_scale=0.0)[0]
    assert torch.equal(open_sky, unshadowed) and not torch.equal(open_sky, shadowed)
    assert (shadowed <= open_sky).all()


def check_shim_random_seed_backward(dev):
    """rnd_seed=None: a seed drawn for the forward and another for the backward; finite gradients of the right shapes"""
    fx = shade_fixture(3)
    ctx = ou.OptiXContext()
    ou.optix_build_bvh(ctx, _to(dev, fx['verts']), _to(dev, fx['tris']), rebuild=1)
    ins = dict(pos=_to(dev, fx['pos'], True), nrm=_to(dev, fx['nrm'], True), kd=_to(dev, fx['kd'], True), ks=_to(dev, fx['ks'], True), light=_to(dev, fx['light'], True))
    diff, spec = ou.optix_env_shade(ctx, _to(dev, fx['mask']), _to(dev, fx['ro']), ins['pos'], ins['nrm'], _to(dev, fx['view']), ins['kd'], ins['ks'], ins['light'],
                                    _to(dev, fx['pdf']), _to(dev, fx['rows']), _to(dev, fx['cols']), n_samples_x=2)
    assert tuple(diff.shape) == tuple(spec.shape) == fx['pos'].shape
    (diff.sum() + spec.sum()).backward()
    for k, v in ins.items():
        assert v.grad is not None and v.grad.shape == v.shape and torch.isfinite(v.grad).all(), k
        assert float(v.grad.abs().max()) > 0, k
    assert (2, str(diff.device)) in ou._random_perm and tuple(ou._random_perm[(2, str(diff.device))].shape) == (32768, 4)


def check_shim_exports():
    assert ou.__all__ == ['OptiXContext', 'optix_build_bvh', 'optix_env_shade', 'bilateral_denoiser']
    ns = {}
    exec('from render.optixutils import *', ns)
    assert sorted(k for k in ns if not k.startswith('__')) == sorted(ou.__all__)
    import inspect
    sig = inspect.signature(ou.optix_env_shade)
    assert list(sig.parameters)[-4:] == ['BSDF', 'n_samples_x', 'rnd_seed', 'shadow_scale']
    assert [sig.parameters[k].default for k in list(sig.parameters)[-4:]] == ['pbr', 8, None, 1.0]
    assert list(inspect.signature(ou.optix_build_bvh).parameters) == ['optix_ctx', 'verts', 'tris', 'rebuild']
    assert list(inspect.signature(ou.bilateral_denoiser).parameters) == ['col', 'nrm', 'zdz', 'sigma']
