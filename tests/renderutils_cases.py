"""Check functions of the BSDF and cube-map entry points of render.renderutils (csrc/bsdf.hip, csrc/cubemap.hip, d3h/bsdf.py, d3h/cubemap.py),
shared by tests/test_renderutils_emul.py (host emulation of the kernel sources) and tests/test_gpu_renderutils.py (MI355X).  Same shapes on
both: the per-pixel cases are the 130 pixels of tests/golden/renderutils_bsdf.npz, the cube maps N in {1, 5, 6, 16} and, for faces of more than
one 16 x 16 patch, N = 20.

Parity rule, everywhere: max|got - f64| / max|f64| <= max(5 * ref32_err, 2^-20) per tensor (output and every gradient), where f64 is the
yardstick in float64 and ref32_err the yardstick's OWN float32 distance from it.  The factor 5 is the project's rule for GPU against oracle
(tests/test_gpu_fullsize.py); the floor is 8 ulp of float32 at the tensor's scale, for functions whose float32 twin is off by one rounding.
  * per-pixel functions: the yardstick is the reference's python twin, recorded by tools/gen_golden_renderutils.py (float64 outputs and
    gradients, and ref32_err of the twin run in float32 on the same inputs);
  * cube maps: the reference's plugin cannot be built without its GPU, so the yardstick is `brute()` below, a float64 numpy evaluation of the
    filters' formulas over ALL texel pairs (no bounds table), and its float32 twin (the same code on float32 arrays) supplies ref32_err.
Every figure is printed before it is asserted (run with -s to see them)."""
import functools
import os

import numpy as np
import torch

import render.renderutils as ru
from render.renderutils import pbr_bsdf  # noqa: F401  (the name whose absence made this an ImportError before the ops existed)
from d3h import bsdf as DB, cubemap as DC

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'renderutils_bsdf.npz')
FLOOR = 2.0 ** -20
MIN_ROUGHNESS = 0.08

# case -> (input names in call order, kernel path / torch composition through the public API)
CASES = {
    'fresnel_shlick': (('f0', 'f90', 'cosTheta'), lambda py, *a: ru._fresnel_shlick(*a, use_python=py)),
    'ndf_ggx': (('alphaSqr', 'cosTheta'), lambda py, *a: ru._ndf_ggx(*a, use_python=py)),
    'lambda_ggx': (('alphaSqr', 'cosTheta'), lambda py, *a: ru._lambda_ggx(*a, use_python=py)),
    'masking_smith': (('alphaSqr', 'cosThetaI', 'cosThetaO'), lambda py, *a: ru._masking_smith(*a, use_python=py)),
    'lambert': (('nrm', 'wi'), lambda py, *a: ru.lambert(*a, use_python=py)),
    'frostbite': (('nrm', 'wi', 'wo', 'linearRoughness'), lambda py, *a: ru.frostbite_diffuse(*a, use_python=py)),
    'pbr_specular': (('col', 'nrm', 'wo', 'wi', 'alpha'), lambda py, *a: ru.pbr_specular(*a, min_roughness=MIN_ROUGHNESS, use_python=py)),
    'pbr_bsdf_lambert': (('kd', 'arm', 'pos', 'nrm', 'view_pos', 'light_pos'), lambda py, *a: ru.pbr_bsdf(*a, min_roughness=MIN_ROUGHNESS, use_python=py)),
    'pbr_bsdf_frostbite': (('kd', 'arm', 'pos', 'nrm', 'view_pos', 'light_pos'),
                           lambda py, *a: ru.pbr_bsdf(*a, min_roughness=MIN_ROUGHNESS, bsdf='frostbite', use_python=py)),
}


@functools.lru_cache(maxsize=None)
def gold():
    g = np.load(GOLD)
    return {k: g[k] for k in g.files}


def bound(case):
    return max(5.0 * float(gold()[f'{case}.ref32_err']), FLOOR)


def rel(got, ref):
    got = got.detach().cpu().double().numpy() if torch.is_tensor(got) else np.asarray(got, np.float64)
    ref = ref.detach().cpu().double().numpy() if torch.is_tensor(ref) else np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.isfinite(got).all()
    return float(np.abs(got - ref).max() / np.abs(ref).max())


def inputs(case, dev, dtype=torch.float32):
    g = gold()
    return {n: torch.from_numpy(g[f'{case}.in.{n}']).to(dev, dtype) for n in CASES[case][0]}


def run(case, dev, ins=None, use_python=False, grad_for=None, dtype=torch.float32):
    """-> (output, {name: gradient or None}) under the golden cotangent"""
    names, fn = CASES[case]
    ins = dict(inputs(case, dev, dtype) if ins is None else ins)
    leaves = {n: ins[n].detach().requires_grad_(grad_for is None or n in grad_for) for n in names}
    out = fn(use_python, *[leaves[n] for n in names])
    gout = torch.from_numpy(gold()[f'{case}.gout']).to(dev, dtype)
    out.backward(gout)
    return out.detach(), {n: leaves[n].grad for n in names}


def assert_close(what, got, ref, tol):
    r = rel(got, ref)
    print(f'{what:48s} {r:.3e}  (bound {tol:.3e}, {r / tol:.2f} of it)')
    assert r <= tol, (what, r, tol)


# ---- per-pixel functions ---------------------------------------------------------------------------------------------------------
def check_parity(dev, case):
    """the kernel path against the reference twin's float64 record: output and every gradient"""
    g = gold()
    out, grads = run(case, dev)
    assert out.dtype == torch.float32
    assert_close(f'{case}: out', out, g[f'{case}.out'], bound(case))
    for n, d in grads.items():
        assert d.shape == g[f'{case}.d.{n}'].shape          # a broadcast input's gradient comes back in the input's own shape
        assert_close(f'{case}: d_{n}', d, g[f'{case}.d.{n}'], bound(case))


def check_python_twin(dev, case):
    """use_python=True (the shim's torch composition, float32 on `dev`) under the same rule as the kernel path: every output and gradient
    against the float64 record.  Both paths being within `bound` of the record, they are within 2 * bound of each other (triangle
    inequality); that figure is printed and held to exactly that, it adds no information of its own."""
    g = gold()
    out_k, grads_k = run(case, dev)
    out_p, grads_p = run(case, dev, use_python=True)
    scale = lambda ref: float(np.abs(ref).max())
    for what, a, b, ref in [('out', out_p, out_k, g[f'{case}.out'])] + [(f'd_{n}', grads_p[n], grads_k[n], g[f'{case}.d.{n}']) for n in grads_k]:
        assert a.shape == b.shape
        assert_close(f'{case}: python {what}', a, ref, bound(case))
        r = float((a - b).abs().max()) / scale(ref)
        print(f'{case}: python - kernel {what:30s} {r:.3e}')
        assert r <= 2.0 * bound(case), (case, what, r)


def _rows(mask):
    m = torch.from_numpy(np.asarray(mask)).reshape(mask.shape[:3])
    assert int(m.sum()) >= 3, 'the fixture no longer holds rows of this kind'
    return m


def check_exact_zeros(dev):
    """masked pixels and clamped parameters get exact zeros; the rows are taken at least 1e-3 away from the switch"""
    g = gold()
    dot = lambda c, a, b: (g[f'{c}.in.{a}'].astype(np.float64) * g[f'{c}.in.{b}'].astype(np.float64)).sum(-1)
    m = 1e-3
    back = {'lambert': dot('lambert', 'wi', 'nrm') < -m,
            'frostbite': (dot('frostbite', 'wi', 'nrm') < -m) | (dot('frostbite', 'wo', 'nrm') < -m),
            'pbr_specular': (dot('pbr_specular', 'wo', 'nrm') < 1e-4 - m) | (dot('pbr_specular', 'wi', 'nrm') < 1e-4 - m)}
    for case, mask in back.items():
        rows = _rows(mask).to(dev)
        out, grads = run(case, dev)
        print(f'{case}: {int(rows.sum())} masked rows')
        for what, t in [('out', out)] + [(f'd_{n}', d) for n, d in grads.items()]:
            assert (t[rows] == 0).all(), (case, what)
    a = g['pbr_specular.in.alpha'][..., 0].astype(np.float64)
    rows = _rows((a < MIN_ROUGHNESS ** 2 - m) | (a > 1.0 + m)).to(dev)
    assert int((torch.from_numpy(a) > 1.0 + m).sum()) >= 3
    _, grads = run('pbr_specular', dev)
    assert (grads['alpha'][rows] == 0).all()
    assert (grads['alpha'][~rows] != 0).any()
    for case, names in (('fresnel_shlick', ('cosTheta',)), ('ndf_ggx', ('cosTheta',)), ('lambda_ggx', ('cosTheta',)),
                        ('masking_smith', ('cosThetaI', 'cosThetaO'))):
        _, grads = run(case, dev)
        for n in names:
            c = g[f'{case}.in.{n}'][..., 0].astype(np.float64)
            lo, hi = _rows(c < 1e-4 - m).to(dev), _rows(c > 1.0 - 1e-4 + m).to(dev)
            assert (grads[n][lo] == 0).all() and (grads[n][hi] == 0).all(), (case, n)
            assert (grads[n][~(lo | hi)] != 0).any()


def check_degenerate_rows_are_finite(dev):
    """pbr_specular with wo = -wi (a zero half vector) and zero-length normals, forward only: finite, and equal to the twin"""
    ins = inputs('pbr_specular', dev)
    ins['wo'][0, 0, :6] = -ins['wi'][0, 0, :6]
    ins['nrm'][0, 0, 3:9] = 0.0
    with torch.no_grad():
        out = ru.pbr_specular(*[ins[n] for n in CASES['pbr_specular'][0]], min_roughness=MIN_ROUGHNESS)
        ref = DB.py_pbr_specular(*[ins[n].cpu().double() for n in CASES['pbr_specular'][0]], min_roughness=MIN_ROUGHNESS)
    assert torch.isfinite(out).all()
    assert (out[0, 0, :9] == 0).all() and (ref[0, 0, :9] == 0).all()
    assert_close('pbr_specular: degenerate rows, out', out, ref, bound('pbr_specular'))


def _py64(case, ins, grad_names):
    """the torch composition in float64 on the CPU: the yardstick for input layouts the fixture does not hold (the composition itself is held
    to the fixture by check_python_twin)"""
    out, grads = run(case, 'cpu', ins={k: v.detach().cpu().double() for k, v in ins.items()}, use_python=True, dtype=torch.float64)
    return out, {n: grads[n] for n in grad_names}


def check_layouts(dev):
    g = gold()
    case = 'pbr_bsdf_lambert'
    # (1) view_pos [2,1,1,3] and light_pos [1,1,1,3] as the fixture has them
    _, grads = run(case, dev)
    assert tuple(grads['view_pos'].shape) == (2, 1, 1, 3) and tuple(grads['light_pos'].shape) == (1, 1, 1, 3)
    assert_close('layout: d_view_pos [2,1,1,3]', grads['view_pos'], g[f'{case}.d.view_pos'], bound(case))
    assert_close('layout: d_light_pos [1,1,1,3]', grads['light_pos'], g[f'{case}.d.light_pos'], bound(case))
    # (2) kd broadcast along the batch
    ins = inputs(case, dev)
    ins['kd'] = ins['kd'][0:1].clone()
    out, grads = run(case, dev, ins=ins)
    ref_out, ref = _py64(case, ins, ('kd', 'arm'))
    assert tuple(grads['kd'].shape) == (1, 5, 13, 3)
    assert_close('layout: kd [1,5,13,3], out', out, ref_out, bound(case))
    assert_close('layout: kd [1,5,13,3], d_kd', grads['kd'], ref['kd'], bound(case))
    assert_close('layout: kd [1,5,13,3], d_arm', grads['arm'], ref['arm'], bound(case))
    # (3) a non-contiguous normal: the same values behind a permuted view
    ins = inputs(case, dev)
    ins['nrm'] = ins['nrm'].permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3)
    assert not ins['nrm'].is_contiguous()
    out, grads = run(case, dev, ins=ins)
    assert_close('layout: permuted nrm, out', out, g[f'{case}.out'], bound(case))
    assert_close('layout: permuted nrm, d_nrm', grads['nrm'], g[f'{case}.d.nrm'], bound(case))
    # (4) the fixture five times along W, 325 pixels per batch item: of the three workgroups of 256 pixels the first and the last lie inside one
    # batch item (gradients of view_pos / light_pos summed in the workgroup), the middle one straddles both (summed per pixel)
    for case in ('pbr_bsdf_lambert', 'pbr_bsdf_frostbite'):
        ins = {k: (v.repeat(1, 1, 5, 1) if v.shape[2] > 1 else v) for k, v in inputs(case, dev).items()}
        names, fn = CASES[case]
        leaves = {n: ins[n].detach().requires_grad_(True) for n in names}
        gout = torch.from_numpy(g[f'{case}.gout']).to(dev).repeat(1, 1, 5, 1)
        fn(False, *[leaves[n] for n in names]).backward(gout)
        ref = {n: ins[n].detach().cpu().double().requires_grad_(True) for n in names}
        fn(True, *[ref[n] for n in names]).backward(gout.cpu().double())
        for n in names:
            assert leaves[n].grad.shape == ins[n].shape
            assert_close(f'layout: {case} at 2 x 5 x 65, d_{n}', leaves[n].grad, ref[n].grad, bound(case))


def check_skipped_gradients(dev):
    """requires_grad on kd alone: the other five gradients are not produced, and kd's is what it was"""
    for case in ('pbr_bsdf_lambert', 'pbr_bsdf_frostbite'):
        _, full = run(case, dev)
        _, only = run(case, dev, grad_for=('kd',))
        assert all(only[n] is None for n in CASES[case][0] if n != 'kd')
        assert torch.equal(only['kd'], full['kd'])


# ---- cube maps -------------------------------------------------------------------------------------------------------------------
CUBE_NS = (1, 5, 6, 16)
# beyond 16 a face is cut into several 16 x 16 patches (the last ones partial), and a workgroup skips the patches its filter cannot reach
CUBE_PATCHED = ((20, 0.08), (20, 0.3), (20, 1.0))
CUBE_ROUGHNESS = (0.08, 0.3, 0.5, 1.0)
CUTOFF = 0.99


@functools.lru_cache(maxsize=None)
def cone_cutoff(roughness, cutoff=CUTOFF):
    """cos(theta) where the running sum of 10^6 samples of the GGX NDF over [0, pi/2] first reaches `cutoff` of its total"""
    c = np.cos(np.linspace(0.0, np.pi / 2.0, 1000000))
    a2 = roughness ** 4
    d = (c * a2 - c) * c + 1.0
    s = np.cumsum(a2 / (d * d * np.pi))
    return float(c[np.argmax(s >= s[-1] * cutoff)])


def texels(N, dt):
    """unit directions [6 N^2, 3] and pixel areas [6 N^2] in texel order [side][y][x], computed in dtype dt"""
    one, half, two = dt(1.0), dt(0.5), dt(2.0)
    idx = np.arange(N).astype(dt)
    f = two * ((idx + half) / dt(N)) - one
    fy, fx = np.meshgrid(f, f, indexing='ij')
    o = np.ones_like(fx)
    sides = [(o, -fy, -fx), (-o, -fy, fx), (fx, o, fy), (fx, -o, -fy), (fx, -fy, o), (-fx, -fy, -o)]
    d = np.stack([np.stack(s, -1) for s in sides]).reshape(-1, 3).astype(dt)
    d = d / np.sqrt((d * d).sum(-1, keepdims=True))
    if N > 1:
        Hh = N // 2
        k = np.abs(np.arange(N) - Hh)
        a1 = (np.arctan((k + 1).astype(dt) / dt(Hh)) - np.arctan(k.astype(dt) / dt(Hh))).astype(dt)
        area = np.tile((a1[:, None] * a1[None, :]).reshape(-1), 6)
    else:
        area = np.ones(6, dt)
    return d.astype(dt), area.astype(dt)


@functools.lru_cache(maxsize=None)
def brute_diffuse(N, dt):
    """diffuse weights Wd [p, q] over all texel pairs, in dtype dt"""
    d, area = texels(N, dt)
    return (np.clip(d @ d.T, dt(0.0), dt(0.999)) * area[None, :] / dt(3.141592)).astype(dt)


@functools.lru_cache(maxsize=4)
def brute(N, roughness, dt):
    """(diffuse weights Wd [p, q], specular weights Ws [p, q], smallest |dot - cutoff|) over all texel pairs, in dtype dt"""
    d, area = texels(N, dt)
    dots = d @ d.T
    Wd = brute_diffuse(N, dt)
    cut = dt(cone_cutoff(roughness))
    inside = dots >= cut
    h = d[:, None, :] + d[None, :, :]
    h = h / np.sqrt(np.maximum((h * h).sum(-1, keepdims=True), dt(1e-20)))
    c = np.clip((d[:, None, :] * h).sum(-1), dt(0.0), dt(1.0))
    a2 = dt(roughness) * dt(roughness)
    a2 = a2 * a2
    dd = (c * a2 - c) * c + dt(1.0)
    ndf = a2 / (dd * dd * dt(np.pi))
    Ws = np.where(inside, np.maximum(dots, dt(0.0)) * ndf * area[None, :] / dt(4.0), dt(0.0)).astype(dt)
    return Wd, Ws, float(np.abs(dots.astype(np.float64) - float(cut)).min())


def brute_eval(N, roughness, cmap, gout, dt):
    Wd, Ws, _ = brute(N, roughness, dt)
    c, g = cmap.reshape(-1, 3).astype(dt), gout.reshape(-1, 3).astype(dt)
    ws = Ws.sum(1, keepdims=True)
    return {'diffuse': Wd @ c, 'd_diffuse': Wd.T @ g, 'specular': (Ws @ c) / ws, 'd_specular': Ws.T @ (g / ws)}


def _cube_inputs(N):
    rng = np.random.default_rng(100 + N)
    return rng.uniform(0.0, 4.0, (6, N, N, 3)).astype(np.float32), rng.standard_normal((6, N, N, 3)).astype(np.float32)


def check_cubemap(dev, N, roughness):
    cmap, gout = _cube_inputs(N)
    r64, r32 = brute_eval(N, roughness, cmap, gout, np.float64), brute_eval(N, roughness, cmap, gout, np.float32)
    inside64, inside32 = brute(N, roughness, np.float64)[1] > 0, brute(N, roughness, np.float32)[1] > 0
    gap = brute(N, roughness, np.float64)[2]
    print(f'N = {N}, roughness {roughness}: cos cutoff {cone_cutoff(roughness):.6f}, smallest |dot - cutoff| {gap:.2e}, '
          f'{int(inside64.sum(1).max())} texels in the largest cone')
    assert (inside64 == inside32).all() and gap > 1e-6          # cone membership is unambiguous in float32: no texel is excluded
    assert DC.costheta_cutoff(N, roughness, CUTOFF) == cone_cutoff(roughness)
    got = {}
    c = torch.from_numpy(cmap).to(dev).requires_grad_(True)
    got['diffuse'] = ru.diffuse_cubemap(c)
    got['diffuse'].backward(torch.from_numpy(gout).to(dev))
    got['d_diffuse'], c.grad = c.grad, None
    got['specular'] = ru.specular_cubemap(c, roughness, cutoff=CUTOFF)
    got['specular'].backward(torch.from_numpy(gout).to(dev))
    got['d_specular'] = c.grad
    for k in ('diffuse', 'd_diffuse', 'specular', 'd_specular'):
        assert tuple(got[k].shape) == (6, N, N, 3) and got[k].dtype == torch.float32
        ref32_err = rel(r32[k], r64[k])
        assert_close(f'cubemap N={N} r={roughness}: {k} (ref32_err {ref32_err:.2e})', got[k].reshape(-1, 3), r64[k], max(5.0 * ref32_err, FLOOR))


def check_cubemap_properties(dev):
    for N in CUBE_NS:
        # roughness 0.08: every cone holds its own texel only, so the filter is the identity
        assert (brute(N, 0.08, np.float64)[1] > 0).sum(1).max() == 1
        cmap, _ = _cube_inputs(N)
        out = ru.specular_cubemap(torch.from_numpy(cmap).to(dev), 0.08)
        assert_close(f'specular_cubemap(c, 0.08) == c at N = {N}', out, cmap, FLOOR)
    # the diffuse filter of an all-ones map is the row sums of the weights
    for N in CUBE_NS:
        rows64, rows32 = brute(N, 0.3, np.float64)[0].sum(1), brute(N, 0.3, np.float32)[0].sum(1)
        if N == 16:
            # pixel_area does not sum to 4 pi (13.594 at N = 16), so the filter of a constant map is not that constant: the row sums lie
            # between 1.046 and 1.116, figures given to three decimals (1.045963 .. 1.115679) and compared at that precision
            print(f'row sums of the diffuse weights at N = 16: {rows64.min():.6f} .. {rows64.max():.6f}')
            assert round(float(rows64.min()), 3) >= 1.046 and round(float(rows64.max()), 3) <= 1.116
        out = ru.diffuse_cubemap(torch.ones(6, N, N, 3, device=dev))
        ref = np.repeat(rows64[:, None], 3, 1)
        assert_close(f'diffuse_cubemap(ones) at N = {N}', out.reshape(-1, 3), ref, max(5.0 * rel(np.repeat(rows32[:, None], 3, 1), ref), FLOOR))


def check_cubemap_backward_is_reproducible(dev, N=16):
    """the gather backward has no atomics: two runs give the same bits"""
    cmap, gout = _cube_inputs(N)
    res = []
    for _ in range(2):
        c = torch.from_numpy(cmap).to(dev).requires_grad_(True)
        (ru.diffuse_cubemap(c) * torch.from_numpy(gout).to(dev)).sum().backward()
        gd, c.grad = c.grad.clone(), None
        (ru.specular_cubemap(c, 0.5) * torch.from_numpy(gout).to(dev)).sum().backward()
        res.append((gd, c.grad.clone()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert res[0][0].abs().max() > 0 and res[0][1].abs().max() > 0


def check_cubemap_validation(dev):
    import pytest
    for shape in ((5, 4, 4, 3), (6, 4, 5, 3), (6, 4, 4, 4)):
        with pytest.raises(RuntimeError):
            ru.diffuse_cubemap(torch.zeros(*shape, device=dev))
        with pytest.raises(RuntimeError):
            ru.specular_cubemap(torch.zeros(*shape, device=dev), 0.3)


def check_patch_cones():
    """host side of the patch skipping: every texel direction of a 16 x 16 patch lies inside the patch's cone (so skipping a patch pair whose
    cones are further apart than the filter reaches drops nothing), for sizes with one, several, full and partial patches per face"""
    for N in (1, 5, 16, 17, 20, 37, 64):
        cones = DC.patch_cones(N)
        d, _ = texels(N, np.float64)
        d = d.reshape(6, N, N, 3)
        ppf = -(-N // DC.PATCH)
        assert cones.shape == (6 * ppf * ppf, 4)
        worst = -1.0
        for t, (ax, ay, az, r) in enumerate(cones):
            side, py, px = t // (ppf * ppf), (t % (ppf * ppf)) // ppf, t % ppf
            patch = d[side, py * 16:(py + 1) * 16, px * 16:(px + 1) * 16].reshape(-1, 3)
            ang = np.arccos(np.clip(patch @ np.array([ax, ay, az]), -1.0, 1.0))
            assert abs(ax * ax + ay * ay + az * az - 1.0) < 1e-12 and len(patch) > 0
            worst = max(worst, float((ang - r).max()))
        print(f'N = {N}: {len(cones)} patches, largest (texel angle - cone angle) {worst:.2e}')
        assert worst <= 0.0
